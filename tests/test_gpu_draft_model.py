"""-m gpu: lossless draft-model speculative decoding (lh_llama_decode_draft; k_draft_model_begin, csrc/kernels_spec.h; the rule is stated in
include/llamahip.h and restated in tests/draft_model_ref.py).

The claim is exactness, so every comparison is == on ids and bytes against a FRESH context of the target model running the resident greedy loop
(lh_llama_decode_greedy): whatever drafts - the target's own weights, its block-int8 or f16 form, another seed, another geometry - the ids and the last
logits are the target's.
 1. drafts; 2. block-int8 and f16 targets; 3. the ends (the window's last position, ragged and one-id runs, a target shape without a multi-row pass);
 4. continuation (two calls = one, and what the other loops produce on both contexts afterwards); 5. the same pair again (another draft_len, another draft
 model behind a freed one, a twin without graphs) with the new kernel once per pass in the route trace; 6. every refusal, after which both contexts still work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llama_go_amd.mlapi import (LH_EINVAL, LH_EUNSUPPORTED, PROMPT, SHAPES, DraftPair, MLError, decode_draft_contexts, decode_greedy_resident,   # noqa: E402
                                make_hparams, route_trace)

pytestmark = pytest.mark.gpu

CTX, N = 64, 40
SMALL = SHAPES["small"]                                                   # vocab 2048, embd 1024, 4 layers
PROMPT8 = [t % SMALL["vocab"] for t in PROMPT]
NARROW = dict(vocab=SMALL["vocab"], embd=256, mult=256, heads=4, layers=2)   # another geometry, the same vocabulary
ODD640 = dict(vocab=515, embd=640, mult=8, heads=5, layers=2)             # tests/eval_route_cases.py: no two-row lm_head, so R is lowered to 1
KERNEL = "k_draft_model_begin"


class Pool:
    """Models by name, and the undisturbed greedy runs of the targets (each from a fresh context), made once."""

    def __init__(self, product):
        self.product, self.models, self.runs = product, {}, {}

    def model(self, name):
        if name not in self.models:
            shape, seed, form = {"f32": (SMALL, 1234, None), "same": (SMALL, 1234, None), "q8": (SMALL, 1234, "q8"), "f16": (SMALL, 1234, "f16"),
                                 "seed": (SMALL, 99, None), "narrow": (NARROW, 1234, None), "odd": (ODD640, 1234, None), "odd2": (ODD640, 5, None),
                                 "tiny": (SHAPES["tiny"], 1234, None)}[name]
            m = self.product.NewSyntheticModel(make_hparams(**shape, ctx=CTX), seed)
            if form == "q8":
                m.QuantizeQ8()
            if form == "f16":
                m.NarrowF16()
            self.models[name] = m
        return self.models[name]

    def prompt(self, name):
        return [t % self.model(name).hp.vocabSize for t in PROMPT8]

    def greedy(self, name, n, prompt=None):
        """(first id behind the prompt, the n ids of the resident loop behind it, its last logits) on a fresh context of model `name`."""
        prompt = prompt or self.prompt(name)
        key = (name, n, tuple(prompt))
        if key not in self.runs:
            c = self.model(name).NewContext(CTX, 1)
            first = int(np.argmax(c.Eval(prompt, 0)))
            ids, lg = decode_greedy_resident(c, first, len(prompt), n, want_logits=True)
            c.free()
            self.runs[key] = (first, ids, lg)
        return self.runs[key]

    def pair(self, target, draft, prompt=None):
        """A pair with the prompt evaluated on both contexts."""
        prompt = prompt or self.prompt(target)
        p = DraftPair(self.model(target), self.model(draft), CTX)
        p.target.Eval(prompt, 0)
        p.draft.Eval(prompt, 0)
        return p

    def close(self):
        for m in self.models.values():
            m.free()


@pytest.fixture(scope="module")
def pool(product):
    p = Pool(product)
    yield p
    p.close()


def check_run(pool, pair, target, n, K, past=8, first=None, rows=None, prompt=None):
    """DecodeDraft of n ids against the target model's own greedy run: ids, last logits byte for byte, and the bookkeeping."""
    g_first, g, lg_last = pool.greedy(target, n, prompt)
    ids, lg, st, tr = pair.DecodeDraft(g_first if first is None else first, past, n, K, want_logits=True)
    assert ids == g, (target, K, ids, g)
    assert lg.tobytes() == lg_last.tobytes(), (target, K, "last logits")
    R = K + 1 if rows is None else rows
    assert st["rows"] == R, st                                   # a silent fall-back to plain steps fails here
    assert st["passes"] == len(tr) and sum(a + 1 for _, a in tr) == n and all(a <= k <= R - 1 for k, a in tr), (st, tr)
    assert st["drafted"] == sum(k for k, _ in tr) and st["accepted"] == sum(a for _, a in tr) and st["empty"] == sum(1 for k, _ in tr if k == 0)
    assert st["passes"] + st["accepted"] == n
    return st, tr


# ---- 1. drafts --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draft", ["same", "q8", "f16", "seed", "narrow"])
def test_every_draft_leaves_the_targets_ids_and_logits(pool, draft):
    pair = pool.pair("f32", draft)
    for K in (1, 3, 7):
        st, tr = check_run(pool, pair, "f32", N, K)
        if draft == "same":      # the draft's steps are the bytes of the target's rows: everything drafted is accepted
            assert st["accepted"] == st["drafted"] and st["passes"] == -(-N // (K + 1)) and all(a == k for k, a in tr), (K, st, tr)
            assert all(k == K for k, _ in tr[:-1])
    pair.free()


# ---- 2. targets -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,draft,Ks", [("q8", "f32", (1, 3)), ("q8", "seed", (3,)), ("f16", "q8", (7,)), ("f16", "f32", (7,))])
def test_block_int8_and_f16_targets(pool, target, draft, Ks):
    pair = pool.pair(target, draft)
    for K in Ks:
        check_run(pool, pair, target, N, K)
    pair.free()


# ---- 3. ends ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draft", ["same", "seed"])
def test_ends_of_the_window_and_of_the_run(pool, draft):
    pair = pool.pair("f32", draft)
    check_run(pool, pair, "f32", CTX - 8, 7)                     # past + n_steps == ctx exactly: the last passes shrink with what is left of the window
    check_run(pool, pair, "f32", CTX - 8, 4)
    for n, K in ((N - 1, 7), (13, 3), (9, 7), (2, 7)):           # n_steps no multiple of R: the last pass is clipped by what remains
        check_run(pool, pair, "f32", n, K)
    st, tr = check_run(pool, pair, "f32", 1, 7)                  # one id: one pass with nothing drafted
    assert tr == [(0, 0)] and st["empty"] == 1
    pair.free()


def test_a_target_shape_without_a_multi_row_pass_takes_plain_steps(pool):
    pair = pool.pair("odd", "odd2")
    st, tr = check_run(pool, pair, "odd", N, 7, rows=1)
    assert st == dict(passes=N, rows=1, drafted=0, accepted=0, empty=N) and tr == [(0, 0)] * N
    # ... and the draft's cache followed: it continues like a fresh context of its model that evaluated the same tokens in one Eval
    first, g, _ = pool.greedy("odd", N)
    twin = pool.model("odd2").NewContext(CTX, 1)
    twin.Eval(pool.prompt("odd"), 0)
    twin.Eval([first] + g[:-1], 8)
    assert pair.draft.GreedyContinue(g[-1], 8 + N, 5) == twin.GreedyContinue(g[-1], 8 + N, 5)
    twin.free()
    pair.free()


# ---- 4. continuation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draft", ["q8", "seed"])
def test_two_calls_equal_one_and_both_contexts_go_on(pool, draft):
    first, g, lg_last = pool.greedy("f32", N)
    pair = pool.pair("f32", draft)
    a, _, _, _ = pair.DecodeDraft(first, 8, 17, 7)
    b, lg, _, _ = pair.DecodeDraft(a[-1], 8 + 17, N - 17, 7, want_logits=True)
    assert a + b == g and lg.tobytes() == lg_last.tobytes()
    # fresh twins that reached the same state by the plain routes
    tt = pool.model("f32").NewContext(CTX, 1)
    tt.Eval(PROMPT8, 0)
    assert decode_greedy_resident(tt, first, 8, N)[0] == g
    td = pool.model(draft).NewContext(CTX, 1)
    td.Eval(PROMPT8, 0)
    for i, t in enumerate([first] + g[:-1]):
        td.Eval([t], 8 + i)
    past = 8 + N
    want = tt.DecodeLookup(g[-1], past, 6, 3, want_logits=True)
    got = pair.target.DecodeLookup(g[-1], past, 6, 3, want_logits=True)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:], "DecodeLookup on the target behind DecodeDraft"
    assert pair.target.GreedyContinue(got[0][-1], past + 6, 4) == tt.GreedyContinue(want[0][-1], past + 6, 4)
    assert pair.draft.GreedyContinue(g[-1], past, 6) == td.GreedyContinue(g[-1], past, 6)
    assert pair.draft.logits().tobytes() == td.logits().tobytes()
    tt.free()
    td.free()
    pair.free()


# ---- 5. again on one pair, another draft behind a freed one, a twin without graphs ----------------------------------------------------------------
def begins(trace, n=None):
    return sum(1 for t in trace if t.startswith(KERNEL + "/") and (n is None or t == f"{KERNEL}/r{n}"))


def test_another_draft_len_another_draft_and_without_graphs(pool, monkeypatch):
    """Every pass enqueues its own kernels (the pass is not a captured graph: DESIGN 3i), so the route trace shows one k_draft_model_begin per pass, all of
    them full-width while the window is far; the loops the two contexts run besides (resident steps, prompt Evals) replay their graphs as ever."""
    pair = pool.pair("f32", "q8")
    (st, _), trace = route_trace(lambda: check_run(pool, pair, "f32", N, 7))
    assert begins(trace) == begins(trace, 8) == st["passes"], (trace, st)
    (st, _), trace = route_trace(lambda: check_run(pool, pair, "f32", N, 3))         # the same pair, another draft_len
    assert begins(trace) == begins(trace, 4) == st["passes"], (trace, st)
    check_run(pool, pair, "f32", N, 7)
    check_run(pool, pair, "f32", N - 3, 7)
    (st, tr), trace = route_trace(lambda: check_run(pool, pair, "f32", CTX - 8, 4))  # up to the window's end: the narrower passes are in the trace as such
    starts = [8 + sum(a + 1 for _, a in tr[:s]) for s in range(len(tr))]             # the position every pass started at, from the (k, a) trace
    widths = [min(5, CTX - p) for p in starts]
    assert begins(trace) == st["passes"] and all(begins(trace, w) == widths.count(w) for w in range(1, 6)), (trace, tr)
    assert widths[-1] < 5 or starts[-1] == CTX - 5, (starts, tr)
    # the draft freed and replaced by a different model on the same target
    for other in ("narrow", "seed", "q8"):
        d = pair.ReplaceDraft(pool.model(other))
        d.Eval(PROMPT8, 0)
        (st, _), trace = route_trace(lambda: check_run(pool, pair, "f32", N, 7))
        assert begins(trace, 8) == st["passes"], (other, trace, st)
    pair.free()
    # a twin whose contexts replay no graph anywhere
    monkeypatch.setenv("LLAMAHIP_NO_GRAPH", "1")                 # (read when a context's plan is made, which is at its first resident call)
    twin = pool.pair("f32", "q8")
    (st, _), trace = route_trace(lambda: check_run(pool, twin, "f32", N, 7))
    monkeypatch.delenv("LLAMAHIP_NO_GRAPH")
    assert begins(trace, 8) == st["passes"], (begins(trace), st)
    check_run(pool, twin, "f32", N, 3)
    twin.free()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(code, match, fn):
    with pytest.raises(MLError, match=match) as e:
        fn()
    assert e.value.code == code, (e.value.code, code, str(e.value))


def twin_run(pool, name):
    """GreedyDecode (prompt Eval + 5 ids through llama.Eval, every step's logits) of a fresh context of model `name`, made once."""
    key = ("twin", name)
    if key not in pool.runs:
        c = pool.model(name).NewContext(CTX, 1)
        pool.runs[key] = c.GreedyDecode(pool.prompt(name), 5)
        c.free()
    return pool.runs[key]


def still_works(pool, ctx, name):
    """The context produces its fresh twin's ids and logits, byte for byte; afterwards it holds the prompt at [0, 8) again."""
    ids, lg = ctx.GreedyDecode(pool.prompt(name), 5)
    want_ids, want_lg = twin_run(pool, name)
    assert ids == want_ids and lg.tobytes() == want_lg.tobytes(), (name, ids, want_ids)


@pytest.mark.parametrize("target", ["f32", "q8"])
def test_refusals_leave_both_contexts_usable(pool, target):
    first, g, _ = pool.greedy(target, N)
    V, kmax = SMALL["vocab"], 3 if target == "q8" else 7
    pair = pool.pair(target, "seed")
    cases = [("itself", lambda: decode_draft_contexts(pair.target, pair.target, first, 8, N, 3)),
             ("draft_len", lambda: pair.DecodeDraft(first, 8, N, 0)),
             ("draft_len", lambda: pair.DecodeDraft(first, 8, N, kmax + 1)),
             ("vocabulary", lambda: pair.DecodeDraft(V, 8, N, 3)),
             ("exceeds the context window", lambda: pair.DecodeDraft(first, 8, CTX - 8 + 1, 3)),
             ("exceeds the context window", lambda: pair.DecodeDraft(first, CTX, 1, 3)),
             ("n_steps", lambda: pair.DecodeDraft(first, 8, 0, 3))]
    for match, fn in cases:                                      # after EACH refusal both contexts of the pair produce their twins' ids and logits
        refused(LH_EINVAL, match, fn)
        still_works(pool, pair.target, target)
        still_works(pool, pair.draft, "seed")
    check_run(pool, pair, target, N, kmax)                       # ... and the very same two contexts then decode the target's run
    # two contexts that do not share a stream
    lone_t, lone_d = pool.model(target).NewContext(CTX, 1), pool.model("seed").NewContext(CTX, 1)
    lone_t.Eval(PROMPT8, 0)
    lone_d.Eval(PROMPT8, 0)
    refused(LH_EINVAL, "different lh_ctx", lambda: decode_draft_contexts(lone_t, lone_d, first, 8, N, 3))
    assert decode_greedy_resident(lone_t, first, 8, N)[0] == g
    still_works(pool, lone_t, target)
    still_works(pool, lone_d, "seed")
    lone_t.free()
    lone_d.free()
    # another vocabulary
    d = pair.ReplaceDraft(pool.model("tiny"))
    d.Eval(pool.prompt("tiny"), 0)
    refused(LH_EINVAL, "vocabularies differ", lambda: pair.DecodeDraft(first, 8, N, 3))
    still_works(pool, pair.target, target)
    still_works(pool, d, "tiny")
    pair.free()


def test_a_layer_shard_on_either_side_is_unsupported(pool, product):
    shard = product.NewSyntheticModel(make_hparams(**SMALL, ctx=CTX), 1234, 0, 1)
    for shard_is_target in (True, False):
        whole = "seed" if shard_is_target else "f32"
        pair = DraftPair(shard, pool.model(whole), CTX) if shard_is_target else DraftPair(pool.model(whole), shard, CTX)
        whole_ctx = pair.draft if shard_is_target else pair.target
        whole_ctx.Eval(PROMPT8, 0)
        refused(LH_EUNSUPPORTED, "whole-model", lambda: pair.DecodeDraft(1, 8, 4, 3))
        still_works(pool, whole_ctx, whole)                      # the whole-model side of the refused pair
        pair.free()
    shard.free()
