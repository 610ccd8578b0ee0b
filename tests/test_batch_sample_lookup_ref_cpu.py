"""The rule of lh_batch_decode_sample_lookup (tests/batch_sample_lookup_ref.py) held to the one-token sampled loop on a toy model, without a GPU: the
logits are a seeded function of the last two tokens, the sampler is tests/sampler_ref.py.  For every row count 1..8 and ring sizes 1, 5 and 64
(ring_size < R included) the simulated loop must give exactly the ids, rings, ring_pos and draws of one-token sampling per pod - with the replay corpus
(everything accepted), with none, and with a replay wrong at every fifth id (partial acceptance)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_lookup_ref as bref           # noqa: E402
import batch_sample_lookup_ref as bsref   # noqa: E402
import feed_sample_ref as fr              # noqa: E402
import sample_lookup_cases as sc          # noqa: E402
import sampler_ref                        # noqa: E402

V, N_STEPS, SEED = 200, 33, 77
SMP = dict(topK=40, topP=0.95, temp=0.8, penalty=1.3)
PROMPTS = [[5, 9, 150, 9], [17, 3, 3, 88, 120, 4], [199, 0, 61]]


def toy_logits(history):
    """a seeded function of the last two tokens"""
    a, b = int(history[-2]), int(history[-1])
    return (np.random.default_rng(1000003 * a + 7919 * b + 11).standard_normal(V) * 4).astype(np.float32)


def sampler(logits, members, draw):
    return sampler_ref.sample(logits, members, seed=SEED, draw=draw, **SMP)[0]


def start(prompt, ring_size):
    """A pod behind its prompt: the ring holds the prompt and the first sampled id, which is pending."""
    pod = fr.Pod(ring_size)
    fr.feed_ring(pod, prompt, fr.FEED_NEW)
    first = fr.sample_step(pod, sampler, toy_logits(prompt))
    return list(prompt) + [first], pod


def tick_runs(ring_size):
    out = []
    for p in PROMPTS:
        w, pod = start(p, ring_size)
        out.append((w, bsref.one_token_loop(w, pod, toy_logits, sampler, N_STEPS), pod))
    return out


def corpora(runs):
    replay = [t for w, ids, _ in runs for t in w + ids]
    bad = list(replay)
    for i in range(5, len(bad), 5):
        bad[i] = (bad[i] + 1) % V
    return dict(replay=replay, none=None, bad=bad)


@pytest.mark.parametrize("ring_size", [1, 5, 64])
@pytest.mark.parametrize("R", range(1, 9))
def test_simulated_loop_equals_one_token_sampling(R, ring_size):
    runs = tick_runs(ring_size)
    for name, corpus in corpora(runs).items():
        pods = [start(p, ring_size)[1] for p in PROMPTS]
        got = bsref.simulate_pods([w for w, _, _ in runs], pods, toy_logits, sampler, N_STEPS, R, 3, 1, corpus, None, V)
        for i, ((ids, trace, stats), (_, want, wpod)) in enumerate(zip(got, runs)):
            assert ids == want, (name, i)
            assert pods[i].key() == wpod.key(), (name, i, "ring, ring_pos and draw")
            assert stats["rows"] == R and stats["passes"] == len(trace) and sum(a + 1 for _, a in trace) == N_STEPS
            assert all(a <= k <= R - 1 for k, a in trace)
        traces = [t for _, t, _ in got]
        assert sum(bref.look_schedule(traces, N_STEPS, max(R, 1))) == bref.batch_passes(traces)
        if R == 1:
            assert all(t == [(0, 0)] * N_STEPS for t in traces)
        if name == "replay" and R > 1:
            assert all(a == k for t in traces for k, a in t), "the run itself as the corpus: every draft is accepted whole"
            assert sum(st["accepted"] for _, _, st in got) > 0
        if name == "bad" and R >= 4:
            assert any(a < k for t in traces for k, a in t), "partial acceptance"


# the passes of the slowest pod, per corpus, at ring size 64: what a loop of R rows costs on this toy run (33 ids per pod)
# replay: every draft is accepted whole, ceil(33 / R); none: the toy run repeats no token, so nothing is ever drafted; bad: in between
PASSES = {
    ("replay", 2): 17, ("replay", 4): 9, ("replay", 8): 5,
    ("none", 2): 33, ("none", 4): 33, ("none", 8): 33,
    ("bad", 2): 22, ("bad", 4): 16, ("bad", 8): 16,
}


def test_pass_counts_are_pinned():
    runs = tick_runs(64)
    got = {}
    for name, corpus in corpora(runs).items():
        for R in (2, 4, 8):
            pods = [start(p, 64)[1] for p in PROMPTS]
            res = bsref.simulate_pods([w for w, _, _ in runs], pods, toy_logits, sampler, N_STEPS, R, 3, 1, corpus, None, V)
            got[(name, R)] = bref.batch_passes([t for _, t, _ in res])
    assert got == PASSES, got
    # bounds that hold for any model: a pass gives 1..R ids
    for (name, R), n in got.items():
        assert -(-N_STEPS // R) <= n <= N_STEPS


def test_ring_view_equals_literal_appends_everywhere():
    rng = np.random.default_rng(5)
    for rs in (1, 2, 5, 8, 64):
        ring = [int(t) for t in rng.integers(1, V, rs)]
        tok = [int(t) for t in rng.integers(1, V, 8)]
        for pos in sorted({0, 1, rs - 1, rs, rs + 1, 3 * rs + 2}):
            for r in range(8):
                assert sorted(sc.ring_view(ring, pos, tok, r)) == sorted(sc.ring_view_literal(ring, pos, tok, r)), (rs, pos, r)


def test_rows_behind_the_draft_are_not_sampled_and_a_finished_pod_commits_nothing():
    w, pod = start(PROMPTS[0], 5)
    tok = [w[-1], 7, 8, w[-1]]
    rows = [toy_logits(w), toy_logits(w + [7]), toy_logits(w + [7, 8])]
    arg = bsref.sample_rows(pod, sampler, rows, tok, 2)
    assert arg[3] == bsref.NOT_SAMPLED and all(a < V for a in arg[:3])
    before = pod.key()
    assert bsref.accept_commit(pod, arg, tok, 2, 10, N_STEPS, N_STEPS, 64)[4] == [] and pod.key() == before
    a, _, _, _, got = bsref.accept_commit(pod, arg, tok, 2, 10, 0, N_STEPS, 64)
    assert got == arg[:a + 1] and pod.ring_pos == before[1] + a + 1 and pod.draw == before[2] + a + 1
