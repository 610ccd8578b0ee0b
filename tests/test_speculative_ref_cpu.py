"""not-gpu: pins tests/speculative_ref.py - the draft rule of include/llamahip.h and the pass-by-pass simulation the GPU tests compare the
device against - on hand cases and on the committed golden greedy ids of the synthetic 7B."""
import json
import os

import pytest

import speculative_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROMPT = [1, 306, 4658, 278, 6593, 310, 2834, 338]
U = ref.UNKNOWN


# ---- the draft rule on hand cases -----------------------------------------------------------------------------------------------------
def test_window_shorter_than_the_ngram_is_skipped():
    assert ref.draft([5], 4, 3, 3) == []                      # n = 1 < G = 3 and nothing smaller allowed
    assert ref.draft([5, 5], 4, 3, 1) == [5]                  # n = 2: G = 3 skipped, G = 2 has no room, G = 1 finds j = 0
    assert ref.draft([7], 4, 1, 1) == []                      # n = G = 1: the only candidate is the suffix itself


def test_the_suffix_may_not_match_itself():
    assert ref.draft([1, 2, 3], 4, 2, 2) == []                # [2, 3] occurs at j = 1 = n - G only
    assert ref.draft([2, 3, 9, 2, 3], 4, 2, 2) == [9, 2, 3]   # j = 0; the continuation may run into the suffix, up to the window's end
    assert ref.draft([4, 4, 4], 4, 2, 2) == [4]               # overlapping: j = 0 <= n - G - 1 = 0, the draft is H[2:3]


def test_largest_j_wins_and_larger_ngram_first():
    H = [1, 2, 7, 1, 2, 8, 1, 2]
    assert ref.draft(H, 2, 2, 1) == [8, 1]                    # [1, 2] at j = 0 and j = 3: the later one
    H = [9, 2, 5, 1, 2, 6, 3, 2, 4, 1, 2]
    assert ref.draft(H, 1, 2, 1) == [6]                       # G = 2 ([1, 2] at j = 3) wins over the later G = 1 match ([2] at j = 7)
    assert ref.draft(H, 1, 1, 1) == [4]


def test_unknown_entries_never_match():
    assert ref.draft([U, 5, U], 4, 1, 1) == []                # the suffix is unknown
    assert ref.draft([3, U, 6, 3, U], 4, 2, 1) == []          # G = 2 and G = 1 suffixes both hold the unknown entry
    assert ref.draft([3, U, 6, 3], 4, 1, 1) == []             # match at j = 0, the continuation starts with an unknown entry: cut in front of it
    assert ref.draft([3, 8, U, 6, 3], 4, 1, 1) == [8]
    assert ref.draft([3, 8, 600, 6, 3], 4, 1, 1, vocab=512) == [8]   # an id outside the vocabulary is unknown to the model


def test_continuation_cut_by_the_windows_end_and_by_the_corpus_end():
    assert ref.draft([1, 2, 3, 1], 7, 1, 1) == [2, 3, 1]
    assert ref.draft([9, 1], 7, 1, 1, corpus=[5, 1, 6, 7]) == [6, 7]
    assert ref.draft([9, 1], 7, 1, 1, corpus=[5, 6, 1]) == []           # j + G < n_corpus: a match at the corpus' last token has no continuation
    assert ref.draft([1, 4, 9, 1], 7, 1, 1, corpus=[1, 6, 7]) == [4, 9, 1]   # the window is searched first


def test_a_corpus_match_only_the_smaller_ngram_finds():
    assert ref.draft([8, 3, 4], 3, 2, 1, corpus=[7, 4, 5, 6]) == [5, 6]     # [3, 4] nowhere; [4] in the corpus only
    assert ref.draft([8, 3, 4], 3, 2, 2, corpus=[7, 4, 5, 6]) == []


def test_limit_clips_the_draft():
    H = [1, 2, 3, 4, 5, 1]
    for limit in range(0, 6):
        assert ref.draft(H, 4, 1, 1, limit=limit) == [2, 3, 4, 5][:min(limit, 4)]


def test_simulation_clips_by_remaining_and_by_the_window():
    win = [1, 2, 3, 1, 2, 3, 1]          # pending 1 at position 6; the greedy continuation is 2 3 1 2 3 ...
    gr = [2, 3, 1] * 10
    tr, st = ref.simulate(win, gr, 6, 3, 2, 1, ctx=64)
    assert tr == [(3, 3), (1, 1)] and st == dict(passes=2, rows=4, drafted=4, accepted=4, empty=0)   # the second pass: remaining - 1 = 1
    # (inside one window position + remaining <= ctx, so remaining - 1 <= ctx - n: the window's end clips only in front of a context swap)
    tr, _ = ref.simulate(win, gr, 12, 3, 2, 1, ctx=9, keep=1)
    # n = 7: limit = ctx - n = 2 -> k = 2; then pending at position 9 = ctx: swap to [1] + the last 4 entries + the pending one again (n = 6)
    assert tr[0] == (2, 2) and ref.swap_window([1, 2, 3, 1, 2, 3, 1, 2, 3, 1], 9, 1) == [1, 1, 2, 3, 1, 1]
    assert sum(a + 1 for _, a in tr) == 12 and all(a <= k for k, a in tr)


def test_swap_window_is_the_reference_swap():
    H = list(range(100, 117))            # ctx = 16, pending = 116
    assert ref.swap_window(H, 16, 0) == list(range(109, 117)) + [116]          # n = 8: seven newest evaluated tokens + pending, pending again
    assert ref.swap_window(H, 16, 4) == [100, 101, 102, 103] + list(range(111, 117)) + [116]
    assert ref.swap_window(H, 16, 15) == list(range(100, 115)) + [116]         # n = 0: nothing re-fed, the pending token at position keep


# ---- the simulation on the committed golden ids (32-layer synthetic 7B, tools/make_golden_ids.py) ----------------------------------------
def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))["ids"]


GOLDEN_CASES = [
    # file, K, replay corpus, passes, drafted, accepted
    ("7b_seed1234_ids.json", 7, False, 95, 79, 4),
    ("7b_seed1234_ids.json", 7, True, 13, 86, 86),
    ("7b_seed1234_int8_ids.json", 3, False, 98, 36, 1),
    ("7b_seed1234_int8_ids.json", 3, True, 25, 74, 74),
]


@pytest.mark.parametrize("name,K,replay,passes,drafted,accepted", GOLDEN_CASES)
def test_simulation_on_the_golden_ids(name, K, replay, passes, drafted, accepted):
    ids = _golden(name)
    tr, st = ref.simulate(PROMPT + [ids[0]], ids[1:100], 99, K, 3, 1, PROMPT + ids if replay else None, ctx=128)
    assert (st["passes"], st["drafted"], st["accepted"]) == (passes, drafted, accepted)
    assert st["rows"] == K + 1 and sum(a + 1 for _, a in tr) == 99 and all(a <= k <= K for k, a in tr)
    assert st["empty"] == sum(1 for k, _ in tr if k == 0)


def test_golden_fp32_without_corpus_breakdown():
    ids = _golden("7b_seed1234_ids.json")
    tr, _ = ref.simulate(PROMPT + [ids[0]], ids[1:100], 99, 7, 3, 1, None, ctx=128)
    drafted = [(k, a) for k, a in tr if k]
    assert len(drafted) == 13
    assert sum(1 for k, a in drafted if a == 0) == 9 and sum(1 for k, a in drafted if 0 < a < k) == 3 and sum(1 for k, a in drafted if a == k) == 1
