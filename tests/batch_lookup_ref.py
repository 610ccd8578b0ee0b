"""lh_batch_decode_lookup (include/llamahip.h) restated in plain Python from the header's text: the choice of R, the window refusal, the accept rule
of one pod in one pass, the per-pod simulation (speculative_ref.simulate with K = R - 1: a pod's trajectory depends on its own ids and window
only), the number of passes the batch runs and the host's look schedule.  No GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speculative_ref as ref   # noqa: E402

PASS_ROWS_MAX = 64


def choose_rows(pods, draft_max, rows_ok, batched=True):
    """R = draft_max + 1, lowered to the largest R with pods * R <= 64 and rows_ok(pods * R) (the predicate behind the feed's sizes_ok); R = 1 needs no
    predicate (plain ticks).  A batch of two or more pods that is not `batched` takes R = 1."""
    if pods > 1 and not batched:
        return 1
    R = int(draft_max) + 1
    while R > 1 and (pods * R > PASS_ROWS_MAX or not rows_ok(pods * R)):
        R -= 1
    return R


def window_ok(past, n_steps, R, ctx):
    """The loop never leaves the window: past[i] + n_steps + R - 1 <= ctx for every pod."""
    return all(int(p) + int(n_steps) + R - 1 <= ctx for p in past)


def accept(arg, tok, k, pos, produced, n_steps, ctx):
    """One pod, one pass of R = len(arg) rows: arg = the rows' greedy ids, tok = [pending, d_1..d_k, filler...].
    -> (a, pos, produced, pending, appended ids).  A finished pod changes nothing."""
    R = len(arg)
    if produced >= n_steps or pos >= ctx:
        return 0, pos, produced, int(tok[0]), []
    k = min(int(k), R - 1)
    a = 0
    while a < k and int(arg[a]) == int(tok[a + 1]):     # fillers never count: only the k drafted rows are compared
        a += 1
    a = min(a, n_steps - produced - 1, ctx - 1 - pos)
    ids = [int(t) for t in arg[:a + 1]]
    return a, pos + a + 1, produced + a + 1, ids[-1], ids


def simulate_pods(windows, greedy, n_steps, R, ngram_max=3, ngram_min=1, corpus=None, ctx=None, vocab=ref.UNKNOWN):
    """windows[i] = pod i's tokens at positions 0..p-1 followed by its pending token; greedy[i] = the n_steps ids pod i produces.
    -> per pod (trace, stats) with stats['rows'] = R."""
    return [ref.simulate(w, g, n_steps, R - 1, ngram_max, ngram_min, corpus, ctx, vocab) for w, g in zip(windows, greedy)]


def batch_passes(traces):
    """The passes the batch runs = those of its slowest pod."""
    return max(len(t) for t in traces)


def look_schedule(traces, n_steps, R):
    """The host's loop: with `low` = the least id count any pod has for certain, it enqueues ceil((n_steps - low) / R) passes, reads every pod's count
    and repeats.  -> the list of run lengths.  Asserts what the header promises: no enqueued pass finds every pod finished."""
    produced = [0] * len(traces)
    at = [0] * len(traces)
    runs, low = [], 0
    while low < n_steps:
        q = -(-(n_steps - low) // R)
        for _ in range(q):
            assert min(produced) < n_steps, "a pass was enqueued that finds every pod finished"
            for i, t in enumerate(traces):
                if produced[i] < n_steps:
                    produced[i] += t[at[i]][1] + 1
                    at[i] += 1
        runs.append(q)
        assert min(produced) >= min(n_steps, low + q)
        low = min(produced)
    assert all(p == n_steps for p in produced) and sum(runs) == batch_passes(traces)
    return runs
