"""The draft-model speculation rule of include/llamahip.h (lh_llama_decode_draft) in plain Python, written from the header's text, over toy "models":
deterministic next-id functions of the token prefix.  A toy model's one-token step at position q reads ITS cache rows [0, q] (row q is the token the
step evaluates) and returns f(those tokens): so the reference also tracks which token every cache row of the target and of the draft holds, and asserts
that every step attends only to rows that hold the committed tokens (and, in front of them, this pass's own draft).  That is what catches a rule
without the draft's extra step, whose cache then misses a row after every fully accepted pass.

decode_draft(..., mutant=...) runs a deliberately wrong rule; check() is the harness the tests hold every run to, and it must report every mutant."""

STALE = -1          # a cache row nothing valid was written to (or a filler step wrote)
MUTANTS = ("no_extra_step", "accept_off_by_one", "limit_ignores_draft_window")


class RuleViolation(AssertionError):
    pass


def greedy(model, window, n_steps):
    """window = the tokens at positions 0..past-1 and the pending token behind them.  -> the n_steps ids of the one-token loop."""
    H, out = [int(t) for t in window], []
    for _ in range(n_steps):
        out.append(int(model(tuple(H))))
        H.append(out[-1])
    return out


class Cache:
    """The rows of one model's KV cache, as the tokens they were computed from."""

    def __init__(self, window, ctx, name):
        self.ctx, self.name = ctx, name
        self.rows = [int(t) for t in window[:-1]] + [STALE] * (ctx - (len(window) - 1))   # the precondition: both caches hold [0, past)

    def step(self, model, token, q, committed, own):
        """One-token step of `model` on this cache: writes row q, attends rows [0, q].  committed = the tokens at [0, pos) everybody agrees on,
        own = this pass's tokens at pos.. up to and including `token`."""
        if not 0 <= q < self.ctx:
            raise RuleViolation(f"{self.name}: a step at position {q} outside its window of {self.ctx}")
        self.rows[q] = int(token)
        want = list(committed) + list(own)
        if self.rows[:q + 1] != want:
            bad = next(i for i in range(q + 1) if self.rows[i] != want[i])
            raise RuleViolation(f"{self.name}: the step at position {q} attends row {bad}, which holds {self.rows[bad]} instead of {want[bad]}")
        return int(model(tuple(self.rows[:q + 1])))

    def filler(self, q):
        if not 0 <= q < self.ctx:
            raise RuleViolation(f"{self.name}: a filler row at position {q} outside its window of {self.ctx}")
        self.rows[q] = STALE


def decode_draft(target, draft, window, n_steps, draft_len, ctx_target, ctx_draft, rows_max=8, mutant=None):
    """The loop of lh_llama_decode_draft.  target / draft: f(prefix tuple) -> id.  window = tokens at 0..past-1 + the pending token.
    -> dict(ids, trace [(k, a)], stats, target_rows, draft_rows).  rows_max: the largest row count the target's shapes carry."""
    assert mutant in (None,) + MUTANTS
    H = [int(t) for t in window]
    past = len(H) - 1
    ctx = ctx_target if mutant == "limit_ignores_draft_window" else min(ctx_target, ctx_draft)
    if past + n_steps > ctx:
        raise ValueError("past + n_steps > ctx: refused")
    R = max(1, min(draft_len + 1, rows_max))
    tc, dc = Cache(H, ctx_target, "target"), Cache(H, ctx_draft, "draft")
    pos, produced, ids, trace = past, 0, [], []
    while produced < n_steps:
        t = H[pos]
        n = min(R, ctx - pos)                                   # near the window's end a narrower pass
        limit = min(ctx - (pos + 1), n_steps - produced - 1)
        k = min(R - 1, limit)
        assert 0 <= k <= n - 1
        e = [t]
        if R > 1:                                               # R = 1: plain greedy steps of the target, no draft work
            last = k - 1 if mutant == "no_extra_step" else k
            for j in range(last + 1):                           # the step j = k is there for the draft's cache row only
                nxt = dc.step(draft, e[j], pos + j, H[:pos], e[:j + 1])
                if j < k:
                    e.append(nxt)
            for j in range(last + 1, n):                        # the device runs a fixed n steps: the ones behind k leave stale rows inside the window
                dc.filler(pos + j)
        else:                                                   # ... but the draft's cache follows (one Eval of the evaluated tokens behind the steps)
            dc.step(draft, t, pos, H[:pos], [t])
        y = [tc.step(target, e[i], pos + i, H[:pos], e[:i + 1]) for i in range(k + 1)]
        for i in range(k + 1, n):
            tc.filler(pos + i)
        a = 0
        while a < k and y[a] == e[a + 1]:
            a += 1
        if mutant == "accept_off_by_one":
            a = min(a + 1, k)
        trace.append((k, a))
        ids += y[:a + 1]
        H += y[:a + 1]
        pos += a + 1
        produced += a + 1
    stats = dict(passes=len(trace), rows=R, drafted=sum(k for k, _ in trace), accepted=sum(a for _, a in trace), empty=sum(1 for k, _ in trace if k == 0))
    return dict(ids=ids, trace=trace, stats=stats, target_rows=tc.rows, draft_rows=dc.rows, window=H)


def check(target, draft, window, n_steps, draft_len, ctx_target, ctx_draft, rows_max=8, mutant=None, perfect=False, never=False):
    """Runs the rule and holds it to what lh_llama_decode_draft promises; returns the run.  Raises AssertionError (RuleViolation included) otherwise.
    perfect / never: the drafter is known to be always / never right, which pins the number of passes."""
    run = decode_draft(target, draft, window, n_steps, draft_len, ctx_target, ctx_draft, rows_max, mutant)
    ids, trace, st = run["ids"], run["trace"], run["stats"]
    past, ctx = len(window) - 1, min(ctx_target, ctx_draft)
    assert ids == greedy(target, window, n_steps), "ids differ from the plain greedy loop"
    assert sum(a + 1 for _, a in trace) == n_steps
    assert st["drafted"] == sum(k for k, _ in trace) and st["accepted"] == sum(a for _, a in trace) and st["accepted"] <= st["drafted"]
    assert all(a <= k <= st["rows"] - 1 for k, a in trace)
    assert st["empty"] == sum(1 for k, _ in trace if k == 0)
    R = st["rows"]
    if perfect and past + n_steps + R <= ctx:                   # the window does not bind
        assert st["passes"] == -(-n_steps // R), (st, n_steps)
    if never and R > 1:
        assert st["passes"] == n_steps, (st, n_steps)
    # the state left behind: both caches hold the evaluated tokens at [0, past + n_steps)
    want = run["window"][:past + n_steps]
    assert run["target_rows"][:past + n_steps] == want, "target cache"
    assert run["draft_rows"][:past + n_steps] == want, "draft cache"
    return run
