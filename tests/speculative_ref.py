"""The lookup-draft rule of include/llamahip.h (lh_lookup_params) and the pass-by-pass simulation of lh_llama_decode_lookup in plain Python,
written from the header's text.  Because the loop's output equals the greedy sequence, the trajectory of (k_s, a_s) is a pure function of the
greedy ids, the window in front of them, the parameters and ctx: the GPU tests compare the device's stats and trace against simulate()."""

UNKNOWN = 0xFFFFFFFF   # a window entry the context does not know: never matches anything


def _last_match(seq, n_j, suffix):
    """The largest j in [0, n_j) with seq[j:j+G] == suffix, or -1."""
    G = len(suffix)
    for j in range(n_j - 1, -1, -1):
        if list(seq[j:j + G]) == suffix:
            return j
    return -1


def draft(window, draft_max, ngram_max=3, ngram_min=1, corpus=None, limit=None, vocab=UNKNOWN):
    """window[-1] is the pending token.  -> the draft ids (at most min(draft_max, limit)).  An id >= vocab is unknown."""
    H = [int(t) for t in window]
    C = [int(t) for t in corpus] if corpus is not None else []
    n, K = len(H), int(draft_max)
    limit = K if limit is None else int(limit)
    for G in range(int(ngram_max), int(ngram_min) - 1, -1):
        if n < G:
            continue
        S = H[n - G:]
        if UNKNOWN in S:
            continue
        j = _last_match(H, n - G, S)                 # j <= n - G - 1: the suffix may not match itself
        if j >= 0:
            d = H[j + G:min(j + G + K, n)]
        else:
            j = _last_match(C, len(C) - G, S)        # j + G < n_corpus: at least one id follows
            if j < 0:
                continue
            d = C[j + G:min(j + G + K, len(C))]
        for i, t in enumerate(d):                    # the draft ends in front of the first unknown entry of its continuation
            if t >= vocab:
                d = d[:i]
                break
        return d[:max(min(len(d), limit), 0)]
    return []


def swap_window(H, ctx, keep):
    """The context swap of the generation loops (server.go:160-172) on a full window H[0..ctx] (H[ctx] = the pending token): the first `keep`
    tokens stay, the last n = (ctx - keep) / 2 entries of H - the pending one among them - are re-fed behind them, and the pending token is
    evaluated once more behind the run."""
    assert len(H) == ctx + 1 and keep < ctx
    n = (ctx - keep) // 2
    return H[:keep] + H[ctx + 1 - n:ctx + 1] + [H[ctx]]


def simulate(window, greedy, n_steps, draft_max, ngram_max=3, ngram_min=1, corpus=None, ctx=None, vocab=UNKNOWN, keep=0):
    """window = the tokens at positions 0..p-1 followed by the pending token at p; greedy[i] = the id the model produces at step i (across
    context swaps, as lh_llama_decode_greedy produces them).  -> (trace [(k_s, a_s)], stats dict).  ctx=None: no window limit."""
    H = [int(t) for t in window]
    produced, trace = 0, []
    while produced < n_steps:
        if ctx is not None and len(H) - 1 >= ctx:
            H = swap_window(H, ctx, keep)
        limit = n_steps - produced - 1
        if ctx is not None:
            limit = min(limit, ctx - len(H))
        d = draft(H, draft_max, ngram_max, ngram_min, corpus, limit, vocab)
        k, a = len(d), 0
        while a < k and int(greedy[produced + a]) == d[a]:
            a += 1
        trace.append((k, a))
        H += [int(t) for t in greedy[produced:produced + a + 1]]
        produced += a + 1
    assert produced == n_steps
    stats = dict(passes=len(trace), rows=draft_max + 1, drafted=sum(k for k, _ in trace), accepted=sum(a for _, a in trace),
                 empty=sum(1 for k, _ in trace if k == 0))
    return trace, stats
