"""lh_batch_decode_sample_lookup (include/llamahip.h) restated in plain Python, composed of pieces that exist: the accept rule of one pod in one pass
(batch_lookup_ref.accept), a pod's sampler state (feed_sample_ref.Pod), the ring view of a row (sample_lookup_cases.ring_view) and the draft rule
(speculative_ref.draft).  A pod's trajectory depends on its own window, ids and sampler state only, so the loop is simulated per pod, over an arbitrary
`logits(history) -> row` function and an arbitrary sampler `sample(row, ring members, draw) -> id`.  No GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_lookup_ref as bref      # noqa: E402
import feed_sample_ref as fr         # noqa: E402
import sample_lookup_cases as sc     # noqa: E402
import speculative_ref as ref        # noqa: E402

NOT_SAMPLED = 0xFFFFFFFF   # arg of a row behind its pod's draft: the sampler leaves it out, the accept step never reads it


def sample_rows(pod, sample, rows, tok, k):
    """The sampler launch for one pod: row r <= k as sampling call pod.draw + r over the ring as if tok[1..r] had been appended; the rows behind the
    draft are not sampled.  rows[r] = the logits of row r.  Nothing of the pod changes."""
    arg = [int(sample(rows[r], sc.ring_view(pod.ring, pod.ring_pos, tok, r), pod.draw + r)) for r in range(k + 1)]
    return arg + [NOT_SAMPLED] * (len(tok) - 1 - k)


def commit(pod, ids):
    """The sampled commit: the accepted ids appended to the pod's ring in order, ring_pos and draw moved on by their number."""
    for t in ids:
        pod.append(t)
    pod.draw += len(ids)


def accept_commit(pod, arg, tok, k, pos, produced, n_steps, ctx):
    """One pod, one pass: batch_lookup_ref.accept, then the commit.  A finished pod commits nothing.  -> what accept returns."""
    res = bref.accept(arg, tok, k, pos, produced, n_steps, ctx)
    commit(pod, res[4])
    return res


def simulate_pod(window, pod, logits, sample, n_steps, R, ngram_max=3, ngram_min=1, corpus=None, ctx=None, vocab=ref.UNKNOWN):
    """window = the pod's tokens at positions 0..p-1 followed by its pending token (which is in the ring already); pod = its sampler state (modified);
    logits(history) = the row behind the last token of `history`.  -> (ids, trace [(k, a)], stats dict with rows = R)."""
    H = [int(t) for t in window]
    lim_ctx = ctx if ctx is not None else len(H) + n_steps + R
    pos, produced, ids, trace = len(H) - 1, 0, [], []
    while produced < n_steps:
        d = ref.draft(H, R - 1, ngram_max, ngram_min, corpus, min(lim_ctx - len(H), n_steps - produced - 1), vocab)
        k = len(d)
        tok = [H[-1]] + d + [H[-1]] * (R - 1 - k)
        rows = [logits(H + d[:r]) for r in range(k + 1)]
        arg = sample_rows(pod, sample, rows, tok, k)
        a, pos, produced, _, got = accept_commit(pod, arg, tok, k, pos, produced, n_steps, lim_ctx)
        trace.append((k, a))
        ids += got
        H += got
    stats = dict(passes=len(trace), rows=R, drafted=sum(k for k, _ in trace), accepted=sum(a for _, a in trace), empty=sum(1 for k, _ in trace if k == 0))
    return ids, trace, stats


def one_token_loop(window, pod, logits, sample, n_steps):
    """What the loop must equal: n_steps sampled ticks of the pod (feed_sample_ref.sample_step per id).  -> ids; pod is modified."""
    H = [int(t) for t in window]
    ids = []
    for _ in range(n_steps):
        t = fr.sample_step(pod, sample, logits(H))
        ids.append(t)
        H.append(t)
    return ids


def simulate_pods(windows, pods, logits, sample, n_steps, R, ngram_max=3, ngram_min=1, corpus=None, ctx=None, vocab=ref.UNKNOWN):
    """Every pod of a batch -> per pod (ids, trace, stats); the passes the batch runs are batch_lookup_ref.batch_passes of the traces."""
    return [simulate_pod(w, p, logits, sample, n_steps, R, ngram_max, ngram_min, corpus, ctx, vocab) for w, p in zip(windows, pods)]
