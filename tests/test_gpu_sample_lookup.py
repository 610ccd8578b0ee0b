"""-m gpu: lossless lookup-draft speculative decoding for SAMPLED generation (lh_sample_rows, lh_llama_decode_sample_lookup; k_sample_rows /
k_sample_small_rows in kernels_sample.h, the commit in k_spec_accept).

The uniforms of the device sampler are counter-based, so the id of sampling call s is a function of the logits row, the lastNTokens ring at that
moment and s.  The claim is therefore exactness and every check is an integer equality:
 A. op level: one multi-row launch == one-token sampling calls in order (the product's own kernel and the checker's SampleTopPTopK), row i as call
    draw0 + i over the ring behind the draft in front of it - shapes x topK x logits kinds x row counts x ring sizes x ring positions, eviction
    and addition cases whose answer differs from the one a kernel that ignores the draft gives, duplicate draft ids, refusals;
 B. loop level: SampleDecodeLookup == SampleDecode of the product and of the checker - single-pass and split attention, fp32 and block-int8,
    replay / no / corrupted corpus, every clipping of the last pass, small rings against a host-stepped loop, a penalty that matters, the window's
    end and two context swaps, the 7B matrix shapes, refusals.  stats and trace == tests/speculative_ref.py's simulation over the known run.
Every loop test asserts stats.rows == draft_max + 1: a silent fall-back to plain steps fails."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_lookup_cases as sc   # noqa: E402
import speculative_ref as ref      # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, MLError, make_hparams, sample_rows   # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("normal", "ties", "flat", "neginf", "zeros")
ROWS = (1, 2, 5, 8)
RINGS = (1, 2, 3, 8, 128)


def ring_positions(rs):
    return (0, rs - 1, rs, 3 * rs + 2)


# ---- A. op level ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs(product, oracle):
    return product.NewContext(1), oracle.NewContext(1)


def one_case(rng, V, kind, rows, rs, pos):
    """Logits rows, a ring with `pos` ids appended and a draft: most ids come from the rows' own top places, where a penalty changes the answer."""
    lg = np.stack([sc.logits_of(rng, V, kind) for _ in range(rows)])
    hot = np.unique(np.argsort(-lg, axis=1, kind="stable")[:, :4])

    def ids(n):
        return [int(hot[rng.integers(0, len(hot))]) if rng.random() < 0.7 else int(rng.integers(0, V)) for _ in range(n)]
    ring, pos = sc.ring_after(ids(pos), rs)
    return lg, ring, pos, [int(rng.integers(0, V))] + ids(rows - 1)


def check_rows(product, oracle, ctxs, lg, ring, pos, tokens, kw, seed, draw0):
    got = [int(t) for t in sample_rows(product, lg, ring, pos, tokens, seed=seed, draw0=draw0, **kw)]
    hctx, octx = ctxs
    want = sc.sequential_ids(lambda l, members, d: product.SampleTopPTopK(hctx, l, members, seed=seed, draw=d, **kw), lg, ring, pos, tokens, draw0)
    assert got == want, ("one-token calls of the product", got, want, len(ring), pos, tokens)
    owant = sc.sequential_ids(lambda l, members, d: oracle.SampleTopPTopK(octx, l, members, seed=seed, draw=d, **kw), lg, ring, pos, tokens, draw0)
    assert got == owant, ("one-token calls of the checker", got, owant, len(ring), pos, tokens)
    return got


SHAPE_CASES = [(V, k) for V in (512, 1000, 32000, 50000) for k in (1, 40, 64, 65, 1024) if k <= V]


@pytest.mark.parametrize("V,topK", SHAPE_CASES)
def test_rows_equal_one_token_calls(product, oracle, ctxs, V, topK):
    """Every kind x every row count, every row count x every ring size, every ring position, both kernels (topK <= 64 or not), both EPT (V <= 32768
    or not), the 4-byte load path (V % 4 != 0: the rows behind the first are not 16-byte aligned)."""
    rng = np.random.default_rng(V * 11 + topK)
    kw = dict(topK=topK, topP=0.95, temp=0.8, repeatPenalty=1.1)
    for i in range(len(KINDS) * len(ROWS)):
        kind, rows, rs = KINDS[i // len(ROWS)], ROWS[i % len(ROWS)], RINGS[i % len(RINGS)]
        pos = ring_positions(rs)[(i + i // 4) % 4]
        lg, ring, pos, tokens = one_case(rng, V, kind, rows, rs, pos)
        check_rows(product, oracle, ctxs, lg, ring, pos, tokens, kw, seed=2024, draw0=int(rng.integers(0, 1000)))


@pytest.mark.parametrize("topK,topP", [(1, 0.95), (40, 0.95), (65, 0.9)])
def test_every_ring_size_position_and_row_count(product, oracle, ctxs, topK, topP):
    """The whole cross of row counts, ring sizes and ring positions at a small vocabulary: passes that wrap the ring and overwrite slots twice
    (ring_size < rows), one slot, a ring that still holds its initial zeros.  With topK = 1 the draft must change the answer of some rows."""
    V = 512
    rng = np.random.default_rng(topK)
    kw = dict(topK=topK, topP=topP, temp=0.8, repeatPenalty=1.3)
    hctx = ctxs[0]
    moved = behind = 0
    for rows in ROWS:
        for rs in RINGS:
            for pos in ring_positions(rs):
                lg, ring, pos, tokens = one_case(rng, V, "normal", rows, rs, pos)
                draw0 = int(rng.integers(0, 1 << 40))
                got = check_rows(product, oracle, ctxs, lg, ring, pos, tokens, kw, seed=7, draw0=draw0)
                if topK == 1:
                    for r in range(1, rows):
                        behind += 1
                        moved += got[r] != product.SampleTopPTopK(hctx, lg[r], ring, seed=7, draw=draw0 + r, **kw)
    assert topK != 1 or moved >= 10, (moved, behind)      # (the checker alone: 19 of 240 rows behind the first answer otherwise)


DET = [(1, 0.95), (65, 0.01)]   # the deterministic settings of both kernels: topK = 1; topK = 65 with a topP that cuts behind the first rank


@pytest.mark.parametrize("V", [512, 1000, 40000])
@pytest.mark.parametrize("topK,topP", DET)
def test_eviction_and_addition_change_the_answer(product, oracle, ctxs, V, topK, topP):
    """Answers a kernel that ignores the draft cannot give.  t is the maximum by a small margin, u the runner-up, c* cold ids."""
    kw = dict(topK=topK, topP=topP, temp=1.0, repeatPenalty=1.5)
    t, u, p = V - 3, 5, 9
    c = [20, 21, 22, 23, 24, 25, 26]
    row = np.full(V, -30.0, np.float32)
    row[t], row[u] = 10.0, 9.9
    rows = 5
    lg = np.stack([row] * rows)
    # eviction: t is a ring member only in the slot the first draft id overwrites - row 0 takes the runner-up, every row behind it t
    for ring, pos in (([t, 30, 31], 3), ([30, t, 31], 4), ([t], 1), ([t], 7), ([30, 31, t], 2)):
        got = check_rows(product, oracle, ctxs, lg, ring, pos, [p] + c[:rows - 1], kw, seed=1, draw0=3)
        assert got == [u] + [t] * (rows - 1), (ring, pos, got)
    # not evicted yet: t sits two slots on, rows 0..2 see it
    assert check_rows(product, oracle, ctxs, lg, [30, 31, t], 3, [p] + c[:rows - 1], kw, seed=1, draw0=3) == [u, u, u, t, t]
    # addition: the draft holds t at index 2 - penalised from row 2 on; a small ring loses it again
    tokens = [p, c[0], t, c[1], c[2]]
    assert check_rows(product, oracle, ctxs, lg, [30] * 128, 128, tokens, kw, seed=1, draw0=0) == [t, t, u, u, u]
    assert check_rows(product, oracle, ctxs, lg, [30] * 128, 5, tokens, kw, seed=1, draw0=0) == [t, t, u, u, u]
    assert check_rows(product, oracle, ctxs, lg, [30, 31], 0, tokens, kw, seed=1, draw0=0) == [t, t, u, u, t]     # slots written twice
    assert check_rows(product, oracle, ctxs, lg, [30], 0, tokens, kw, seed=1, draw0=0) == [t, t, u, t, t]
    # the initial zeros of a ring that is not full yet keep token 0 a member: with 0 as the maximum every row takes the runner-up
    row0 = row.copy()
    row0[0], row0[t] = 10.0, -30.0
    lg0 = np.stack([row0] * rows)
    assert check_rows(product, oracle, ctxs, lg0, [30, 0, 0, 0, 0, 0, 0, 0], 1, [p] + c[:rows - 1], kw, seed=1, draw0=0) == [u] * rows
    assert check_rows(product, oracle, ctxs, lg0, [30, 0, 0, 0], 1, [p] + c[:rows - 1], kw, seed=1, draw0=0) == [u, u, u, 0, 0]   # the last zero leaves with row 3's appends


@pytest.mark.parametrize("topK,topP", DET)
def test_duplicate_draft_ids(product, oracle, ctxs, topK, topP):
    V, t, u = 1000, 700, 5
    kw = dict(topK=topK, topP=topP, temp=1.0, repeatPenalty=1.5)
    row = np.full(V, -30.0, np.float32)
    row[t], row[u] = 10.0, 9.9
    lg = np.stack([row] * 5)
    tokens = [9, t, t, 20, 21]
    assert check_rows(product, oracle, ctxs, lg, [30], 0, tokens, kw, seed=1, draw0=0) == [t, u, u, t, t]          # one slot: gone with the append behind the pair
    assert check_rows(product, oracle, ctxs, lg, [30, 31], 0, tokens, kw, seed=1, draw0=0) == [t, u, u, u, t]      # both slots held it
    assert check_rows(product, oracle, ctxs, lg, [30, 31, 32], 1, tokens, kw, seed=1, draw0=0) == [t, u, u, u, u]
    rng = np.random.default_rng(3)
    for rs in RINGS:
        lg, ring, pos, tokens = one_case(rng, V, "normal", 8, rs, rs)
        tokens[3] = tokens[1]
        tokens[7] = tokens[6]
        check_rows(product, oracle, ctxs, lg, ring, pos, tokens, dict(topK=40, topP=0.95, temp=0.8, repeatPenalty=1.3), seed=4, draw0=11)


def test_sample_rows_refusals(product):
    V = 1000
    lg = np.zeros((2, V), np.float32)
    good = dict(topK=40, topP=0.95, temp=0.8, repeatPenalty=1.1)
    assert len(sample_rows(product, lg, [1, 2], 2, [V + 5, 3], **good)) == 2               # tokens[0] is ignored, whatever it holds
    with pytest.raises(MLError, match="rows"):
        sample_rows(product, np.zeros((0, V), np.float32), [1], 0, [], **good)
    with pytest.raises(MLError, match="rows"):
        sample_rows(product, np.zeros((9, V), np.float32), [1], 0, [0] * 9, **good)
    with pytest.raises(MLError, match="vocabulary"):
        sample_rows(product, np.zeros((1, 0), np.float32), [1], 0, [0], **good)
    with pytest.raises(MLError, match="vocabulary"):
        sample_rows(product, np.zeros((1, 65537), np.float32), [1], 0, [0], **good)
    with pytest.raises(MLError, match="slot"):
        sample_rows(product, lg, [], 0, [0, 1], **good)
    with pytest.raises(MLError, match="draft id"):
        sample_rows(product, lg, [1], 0, [0, V], **good)
    for bad, msg in ((dict(topK=0), "topK"), (dict(topK=V + 1), "topK"), (dict(temp=0.0), "temp"), (dict(repeatPenalty=0.0), "repeatPenalty")):
        with pytest.raises(MLError, match=msg):
            sample_rows(product, lg, [1], 0, [0, 1], **dict(good, **bad))
    with pytest.raises(MLError, match="device limit"):
        sample_rows(product, np.zeros((1, 4000), np.float32), [1], 0, [0], **dict(good, topK=2000))
    # null arguments, straight at the entry point
    f = product.lib.llamago_SampleRows
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    one, out = (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 8)()
    args = [lg.ctypes.data_as(f32p), 2, V, C.cast(one, u32p), 2, 0, C.cast(one, u32p), 40, 0.95, 0.8, 1.1, 1, 0, C.cast(out, u32p)]
    assert f(*args) == 0
    for i in (0, 3, 6, 13):
        a = list(args)
        a[i] = None
        assert f(*a) != 0 and b"null" in product.lib.ml_LastError(), i


# ---- B. loop level --------------------------------------------------------------------------------------------------------------------------
class Pool:
    """Models and undisturbed sampled runs, made once."""

    def __init__(self, product, oracle):
        self.product, self.oracle, self.models, self.runs = product, oracle, {}, {}

    def hparams(self, name, ctx):
        return make_hparams(**(sc.HD128 if name == "hd128" else dict(SHAPES["7B"], layers=2)), ctx=ctx)

    def model(self, name, ctx, int8):
        key = (name, ctx, int8)
        if key not in self.models:
            m = self.product.NewSyntheticModel(self.hparams(name, ctx), sc.MODEL_SEED)
            if int8:
                m.QuantizeQ8()
            self.models[key] = m
        return self.models[key]

    def sampled(self, name, ctx, int8, prompt, n, seed, keep=0, **smp):
        """(ids of the product's SampleDecode - equal to the checker's -, logits of one more Eval behind the run or None)."""
        key = (name, ctx, int8, tuple(prompt), n, seed, keep, tuple(sorted(smp.items())))
        if key not in self.runs:
            c = self.model(name, ctx, int8).NewContext(ctx, 1)
            c.SetKeepCount(keep)
            run = c.SampleDecode(prompt, n, seed=seed, **smp)
            more = c.Eval([run[-1]], len(prompt) + n - 1) if len(prompt) + n - 1 < ctx else None
            c.free()
            om = self.oracle.NewSyntheticModel(self.hparams(name, ctx), sc.MODEL_SEED)
            if int8:
                om.QuantizeQ8()
            oc = om.NewContext(ctx, 16)
            oc.SetKeepCount(keep)
            orun = oc.SampleDecode(prompt, n, seed=seed, **smp)
            oc.free()
            om.free()
            assert run == orun, "the product's SampleDecode and the checker's"
            self.runs[key] = (run, more)
        return self.runs[key]

    def close(self):
        for m in self.models.values():
            m.free()


@pytest.fixture(scope="module")
def pool(product, oracle):
    p = Pool(product, oracle)
    yield p
    p.close()


def run_lookup(pool, name, ctx, int8, prompt, n, K, corpus, seed=sc.LOOP_SEEDS[0], keep=0, gmax=3, gmin=1, stats_exact=True, smp=sc.SMP):
    """SampleDecodeLookup against the undisturbed SampleDecode of the same settings.  corpus: None, a list, or "replay" / "corrupted" (from the run)."""
    run, more = pool.sampled(name, ctx, int8, prompt, n, seed, keep, **smp)
    if corpus == "replay":
        corpus = list(prompt) + run
    elif corpus == "corrupted":
        corpus = sc.corrupted(list(prompt) + run, len(prompt), pool.model(name, ctx, int8).hp.vocabSize)
    c = pool.model(name, ctx, int8).NewContext(ctx, 1)
    c.SetKeepCount(keep)
    ids, st, tr = c.SampleDecodeLookup(prompt, n, K, gmax, gmin, corpus, seed=seed, **smp)
    assert st["rows"] == K + 1, st
    assert ids == run, (ids, run)
    assert st["passes"] == len(tr) <= max(n - 1, 0) and all(a <= k <= K for k, a in tr) and sum(a + 1 for _, a in tr) == n - 1
    assert st["drafted"] == sum(k for k, _ in tr) and st["accepted"] == sum(a for _, a in tr) and st["empty"] == sum(1 for k, _ in tr if k == 0)
    if stats_exact:   # the accept rule over a known run is the function the greedy loop's simulation states
        vocab = pool.model(name, ctx, int8).hp.vocabSize
        want_tr, want_st = ref.simulate(list(prompt) + [run[0]], run[1:], n - 1, K, gmax, gmin, corpus, ctx, vocab, keep)
        assert tr == want_tr and st == want_st, (tr, want_tr)
    if more is not None:   # the state left behind: one more Eval gives what it gives behind SampleDecode
        again = c.Eval([ids[-1]], len(prompt) + n - 1)
        assert (again.tobytes() == more.tobytes()) if not int8 else (int(np.argmax(again)) == int(np.argmax(more)))
    assert c.SampleDecode(prompt, n, seed=seed, **smp) == run, "a plain sampled run on the same context afterwards"
    c.free()
    return st, tr


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
@pytest.mark.parametrize("ctx", [256, 384])
def test_loop_equals_sample_decode(pool, ctx, int8):
    K, n, V = sc.kmax(int8), sc.N_PREDICT, sc.HD128["vocab"]
    prompt = sc.prompt_for(V, 8)
    st, tr = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, "replay")
    assert st["accepted"] > 0 and st["passes"] < n - 1, st
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, None)
    st, tr = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, "corrupted", gmax=2)
    assert any(a < k for k, a in tr), tr
    for steps in (1, 2, 3, 4, K + 3, 2 * K + 4):                                          # the last pass clipped by what remains
        run_lookup(pool, "hd128", ctx, int8, prompt, steps, K, "replay")
    other = sc.LOOP_SEEDS[1]
    assert pool.sampled("hd128", ctx, int8, prompt, n, other, **sc.SMP)[0] != pool.sampled("hd128", ctx, int8, prompt, n, sc.LOOP_SEEDS[0], **sc.SMP)[0]
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, "replay", seed=other)
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, "corrupted", seed=other, gmax=2)


def test_loop_without_captured_graphs(pool, monkeypatch):
    monkeypatch.setenv("LLAMAHIP_NO_GRAPH", "1")
    prompt = sc.prompt_for(sc.HD128["vocab"], 8)
    run_lookup(pool, "hd128", 256, False, prompt, sc.N_PREDICT, 7, "replay")
    run_lookup(pool, "hd128", 256, False, prompt, sc.N_PREDICT, 7, "corrupted", gmax=2)


@pytest.mark.parametrize("topK", [40, 100], ids=["k40", "k100"])
@pytest.mark.parametrize("ring_size", [1, 5])
def test_small_rings_against_a_host_stepped_loop(pool, product, ring_size, topK):
    """A ring smaller than a pass: every pass overwrites slots more than once.  Baseline: Eval of one token, then the product's one-token sampler over a
    host-kept ring with draw = s (fp32: one-token Evals are byte-equal to resident steps).  topK 100 takes the loop through k_sample_rows."""
    ctx, K, n, seed = 256, 7, 32, 99
    smp = dict(sc.SMP, topK=topK)
    prompt = sc.prompt_for(sc.HD128["vocab"], 8)
    model = pool.model("hd128", ctx, False)
    hctx = product.NewContext(1)
    c = model.NewContext(ctx, 1)
    ring, pos = sc.ring_after(prompt, ring_size)
    lg, want = c.Eval(prompt, 0), []
    for s in range(n):
        tok = int(product.SampleTopPTopK(hctx, lg, ring, seed=seed, draw=s, **smp))
        ring[pos % ring_size] = tok
        pos += 1
        want.append(tok)
        if s + 1 < n:
            lg = c.Eval([tok], len(prompt) + s)
    for corpus in (list(prompt) + want, None, sc.corrupted(list(prompt) + want, len(prompt), sc.HD128["vocab"])):
        ids, st, tr = c.SampleDecodeLookup(prompt, n, K, 3, 1, corpus, ring_size=ring_size, seed=seed, **smp)
        assert ids == want and st["rows"] == K + 1, (ids, want, st)
        want_tr, want_st = ref.simulate(list(prompt) + [want[0]], want[1:], n - 1, K, 3, 1, corpus, ctx, sc.HD128["vocab"])
        assert tr == want_tr and st == want_st
    c.free()


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_the_penalty_matters(pool, int8):
    K, n = sc.kmax(int8), sc.N_PREDICT
    prompt = sc.prompt_for(sc.HD128["vocab"], 8)
    hard, soft = dict(sc.SMP, topK=1, repeatPenalty=1.5), dict(sc.SMP, topK=1, repeatPenalty=1.0)
    run_lookup(pool, "hd128", 256, int8, prompt, n, K, "replay", smp=hard)
    run_lookup(pool, "hd128", 256, int8, prompt, n, K, "corrupted", gmax=2, smp=hard)
    assert pool.sampled("hd128", 256, int8, prompt, n, sc.LOOP_SEEDS[0], **hard)[0] != pool.sampled("hd128", 256, int8, prompt, n, sc.LOOP_SEEDS[0], **soft)[0]


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_loop_clipped_by_the_window_then_swaps(pool, int8):
    """A start 13 positions in front of the window's end: the passes there shrink with what is left of the window, then the context swaps as
    SampleDecode does (the ring is not touched by a swap) and full passes go on."""
    ctx, keep, K, n = 256, 8, sc.kmax(int8), 40
    prompt = sc.prompt_for(sc.HD128["vocab"], ctx - 13, seed=11)
    st, _ = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, "replay", keep=keep)
    assert st["accepted"] > 0
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, None, keep=keep)


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_loop_across_two_context_swaps(pool, int8):
    ctx, keep, K, n = 64, 8, sc.kmax(int8), 101     # from position 8: the first swap after 56 ids, the second 28 later; the ring of 64 evicts from id 57 on
    prompt = sc.prompt_for(sc.HD128["vocab"], 8)
    st, _ = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, "replay", keep=keep, stats_exact=False)
    assert st["accepted"] > 0 and st["passes"] < n - 1
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, None, keep=keep, stats_exact=False)


def test_loop_on_the_7b_matrix_shapes(pool):
    st, _ = run_lookup(pool, "7b", 64, False, PROMPT, 16, 7, "replay")
    assert st["accepted"] > 0


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_refusals_and_the_run_behind_them(pool, product, int8):
    ctx, n = 256, 12
    V, K = sc.HD128["vocab"], sc.kmax(int8)
    prompt = sc.prompt_for(V, 8)
    run, _ = pool.sampled("hd128", ctx, int8, prompt, n, 99, **sc.SMP)
    c = pool.model("hd128", ctx, int8).NewContext(ctx, 1)
    assert c.SampleDecodeLookup(prompt, n, K, seed=99, **sc.SMP)[0] == run
    for kw in (dict(draft_max=0), dict(draft_max=K + 1), dict(draft_max=K, ngram_min=0), dict(draft_max=K, ngram_max=2, ngram_min=3),
               dict(draft_max=K, ngram_max=9), dict(draft_max=K, corpus=[1] * 65537), dict(draft_max=K, corpus=[1, 2, V, 3])):
        with pytest.raises(MLError):
            c.SampleDecodeLookup(prompt, n, seed=99, **dict(sc.SMP, **kw))
    for bad, msg in ((dict(topK=0), "topK"), (dict(topK=V + 1), "topK"), (dict(temp=0.0), "temp"), (dict(repeatPenalty=0.0), "repeatPenalty")):
        with pytest.raises(MLError, match=msg):
            c.SampleDecodeLookup(prompt, n, K, seed=99, **dict(sc.SMP, **bad))
    with pytest.raises(MLError, match="exceeds the context window"):
        c.SampleDecodeLookup([1] * (ctx + 1), n, K, seed=99, **sc.SMP)
    with pytest.raises(MLError):
        c.SampleDecodeLookup([], n, K, seed=99, **sc.SMP)
    with pytest.raises(MLError):
        c.SampleDecodeLookup(prompt, 0, K, seed=99, **sc.SMP)
    # ring_size: 0 is the reference's ring of ctxSize ids; another size is another ring (here it changes the run: token 0 and the prompt leave it)
    assert c.SampleDecodeLookup(prompt, n, K, ring_size=ctx, seed=99, **sc.SMP)[0] == run
    assert c.SampleDecode(prompt, n, seed=99, **sc.SMP) == run, "the context samples what it would have sampled"
    assert c.SampleDecodeLookup(prompt, n, K, seed=99, **sc.SMP)[0] == run
    c.free()
    shard = product.NewSyntheticModel(make_hparams(**sc.HD128, ctx=ctx), sc.MODEL_SEED, 0, 1)
    s2 = shard.NewContext(ctx, 1)
    with pytest.raises(MLError, match="whole-model"):
        s2.SampleDecodeLookup([1, 2], 4, K, seed=99, **sc.SMP)
    s2.free()
    shard.free()
