"""not-gpu: the host-side rules of lh_batch_decode_lookup as tests/batch_lookup_ref.py restates them - the choice of R, the window refusal, the accept
rule, the pass count and the look schedule."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_lookup_ref as bref   # noqa: E402
import speculative_ref as ref     # noqa: E402


def test_rows_times_pods_never_exceed_a_pass():
    for P in range(1, 65):
        for dm in range(1, 8):
            R = bref.choose_rows(P, dm, lambda n: True)
            assert 1 <= R <= dm + 1 and (R == 1 or P * R <= 64), (P, dm, R)
            assert R == max(1, min(dm + 1, 64 // P)), (P, dm, R)
            assert bref.choose_rows(P, dm, lambda n: True, batched=False) == (R if P == 1 else 1)
    assert bref.choose_rows(8, 7, lambda n: True) == 8 and bref.choose_rows(9, 7, lambda n: True) == 7
    assert bref.choose_rows(33, 7, lambda n: True) == 1 and bref.choose_rows(64, 1, lambda n: True) == 1


def test_rows_are_lowered_when_a_size_is_not_ok():
    assert bref.choose_rows(4, 7, lambda n: n != 32) == 7
    assert bref.choose_rows(4, 7, lambda n: n not in (32, 28, 24)) == 5
    assert bref.choose_rows(3, 3, lambda n: False) == 1                      # nothing ok: plain ticks, whatever the predicate says about 3 rows
    assert bref.choose_rows(2, 1, lambda n: n <= 4) == 2 and bref.choose_rows(2, 3, lambda n: n <= 4) == 2
    asked = []
    bref.choose_rows(5, 7, lambda n: asked.append(n) or n == 20)
    assert asked == [40, 35, 30, 25, 20]                                     # only multiples of P, never more than 64, from the top


def test_window_refusal_boundary():
    ctx, R, n = 256, 4, 40
    edge = ctx - n - R + 1
    assert bref.window_ok([edge], n, R, ctx) and bref.window_ok([0, edge], n, R, ctx)
    assert not bref.window_ok([edge + 1], n, R, ctx) and not bref.window_ok([0, edge + 1], n, R, ctx)
    assert edge + n + R - 1 == ctx
    assert bref.window_ok([ctx - n], n, 1, ctx) and not bref.window_ok([ctx - n + 1], n, 1, ctx)   # R = 1: lh_batch_decode's own window, no swap


def test_accept_rule():
    tok = [9, 1, 2, 3, 9, 9, 9, 9]                                           # pending 9, draft 1 2 3, filler
    assert bref.accept([1, 2, 3, 4, 0, 0, 0, 0], tok, 3, 10, 0, 40, 64) == (3, 14, 4, 4, [1, 2, 3, 4])
    assert bref.accept([1, 2, 3, 9, 7, 0, 0, 0], tok, 3, 10, 0, 40, 64)[0] == 3     # a filler row that "matches" never counts
    assert bref.accept([5, 2, 3, 4, 0, 0, 0, 0], tok, 3, 10, 0, 40, 64) == (0, 11, 1, 5, [5])
    assert bref.accept([1, 3, 3, 4, 0, 0, 0, 0], tok, 3, 10, 0, 40, 64) == (1, 12, 2, 3, [1, 3])   # the wrong entry is a later continuation
    assert bref.accept([1, 2, 3, 4, 0, 0, 0, 0], tok, 3, 10, 38, 40, 64) == (1, 12, 40, 2, [1, 2])  # clipped by remaining - 1
    assert bref.accept([1, 2, 3, 4, 0, 0, 0, 0], tok, 3, 62, 0, 40, 64) == (1, 64, 2, 2, [1, 2])    # clipped by the window
    assert bref.accept([1, 2, 3, 4, 0, 0, 0, 0], tok, 3, 10, 40, 40, 64) == (0, 10, 40, 9, [])      # finished: nothing changes
    assert bref.accept([7], [9], 5, 10, 0, 40, 64) == (0, 11, 1, 7, [7])                            # R = 1


def _random_traces(rng, pods, n_steps, R):
    traces = []
    for _ in range(pods):
        t, produced = [], 0
        while produced < n_steps:
            k = int(rng.integers(0, R))
            a = min(int(rng.integers(0, k + 1)), n_steps - produced - 1)
            t.append((k, a))
            produced += a + 1
        traces.append(t)
    return traces


def test_look_schedule_never_enqueues_a_pass_for_finished_pods():
    rng = np.random.default_rng(5)
    for R in (2, 4, 7, 8):
        for n in (1, 2, R, R + 1, 41, 100):
            full = [(R - 1, min(R - 1, n - 1 - s)) for s in range(0, n, R)]              # every pass accepts all it may
            slow = [(0, 0)] * n                                                          # every draft empty
            for traces in [[full], [slow], [full, slow], [slow, full, full]] + [_random_traces(rng, int(rng.integers(1, 9)), n, R) for _ in range(20)]:
                runs = bref.look_schedule(traces, n, R)                                  # (asserts inside)
                assert sum(runs) == bref.batch_passes(traces) and runs[0] == -(-n // R)
            assert bref.look_schedule([full], n, R) == [-(-n // R)]                       # full acceptance: one run, one look


def test_pod_simulation_is_the_solo_rule_per_pod():
    g0 = [5, 6, 7, 5, 6, 7, 5, 6, 7, 5, 6, 7]
    g1 = [1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14, 15]
    w0, w1 = [5, 6, 7, 5], [20, 21, 22]
    got = bref.simulate_pods([w0, w1], [g0[1:], g1], 11, 4, ctx=64)
    assert got[0] == ref.simulate(w0, g0[1:], 11, 3, ctx=64) and got[1] == ref.simulate(w1, g1, 11, 3, ctx=64)
    assert got[0][1]["rows"] == 4 and got[0][1]["accepted"] > 0 and got[1][1]["accepted"] == 0
    assert bref.batch_passes([t for t, _ in got]) == len(got[1][0]) == 11
