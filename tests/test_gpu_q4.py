"""gpu: block-int4 weight matrices (dtype 2 = ml.TYPE_Q4_0; csrc/kernels_q4.h) - every comparison is == on bytes or ids, no tolerance anywhere.

The reference of every model test is the same.  Model A is a synthetic model quantised with QuantizeQ4; model B is the same seed through QuantizeQ4 and
then ExpandQ4: a block-int8 model with the same quants and the same scales, which runs only the int8 kernels the rest of the suite holds to the checker
and to float64 bounds.  A 4-bit quant q in [-8, 7] with scale d IS an int8 weight with the same q and d, so A and B hold identical values and whatever A
computes has to be B's bytes: on the 4-bit forms of the decode stream (one row, 2..4 rows), which keep the int8 kernels' lane -> column map and
summation order, and on every other route, where A runs B's kernels over an int8 image."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import node_path_abi as NP            # noqa: E402
import q4_ref as Q                    # noqa: E402
import weight_probe_ref as WP         # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, DraftPair, MLError, decode_greedy_resident, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
LH_EINVAL, LH_EUNSUPPORTED = -1, -4
Q4_KERNELS = ("k_gemv_q4s", "k_gemv_q4_rows", "k_expand_q4")
# (The int8 decode launches k_gemv_q8s / k_gemv_q8_rows have no route-trace entry - launch_gemv_q8 and launch_gemv_q8_rows of csrc/plan.hip record nothing -
# so a trace cannot show that A stays off them, nor tell A's one-row lm_head on k_gemv_q4s from B's on k_gemv_q8s.  What holds A to its own kernels is
# the positive side: the Q4 names that must appear per route, and the bytes.)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def families(trace):
    """kernel names of a route trace without template arguments and suffixes: 'k_gemv_q4s<1,8,256,256>' -> 'k_gemv_q4s'"""
    return [e.split("<")[0].split("/")[0] for e in trace]


def fused(product, c):
    product.lib.llamago_LastGraphFused.restype = C.c_int
    product.lib.llamago_LastGraphFused.argtypes = [C.c_void_p]
    product.lib.llama_MLContext.restype = C.c_void_p
    return product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h))


def twins(product, hp, seed=77):
    """(A, B): the same synthetic values as block-int4 and as the block-int8 expansion of those very blocks"""
    out = []
    for expand in (False, True):
        m = product.NewSyntheticModel(hp, seed)
        assert m.weight_type == 0
        m.QuantizeQ4()
        assert m.weight_type == 2
        if expand:
            m.ExpandQ4()
            assert m.weight_type == 7
        out.append(m)
    return out


poisoned = WP.poisoned


def seeded_cache(ctxs, hp, layers, ctx):
    """the same seeded finite values in the K and V caches of every context: rows below `past` that no Eval of the test wrote"""
    rng = np.random.default_rng(5)
    n = layers * ctx * hp.embdSize
    for which in (0, 1):
        v = (rng.standard_normal(n) * 0.5).astype(np.float32)
        for c in ctxs:
            c.CacheWrite(which, 0, v)


# ---- 1. quantiser and conversions, op level ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip(product):
    import llama_go_amd as pkg
    lib = NP.bind(C.CDLL(pkg.LIBLLAMAHIP))
    lib.lh_buf_quantize_q4.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.lh_buf_expand_q4.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.lh_buf_quantize_q8.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.lh_buf_narrow_f16.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.lh_buf_upload.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, NP.F32P, C.c_uint64]
    lib.lh_buf_fill_synth.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_float, C.c_float]
    lib.lh_buf_read_q4.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.lh_buf_nfloats.restype = C.c_uint64
    lib.lh_buf_nfloats.argtypes = [C.c_void_p, C.c_uint64]
    return lib


@pytest.fixture()
def sess(hip):
    s = NP.Session(hip)
    yield s
    s.close()


def new_buf(s, fn, *args):
    out = C.c_uint64()
    rc = fn(s.ctx, *args, C.byref(out))
    if rc == 0:
        s.bufs.append(out.value)
    return rc, out.value


def register_q4(s, raw, rows, cols):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    assert raw.size == rows * cols // 32 * 20
    ne = (C.c_uint32 * 4)(cols, rows, 1, 1)
    buf = C.c_uint64()
    assert s.lib.lh_tensor_register(s.ctx, 0, 2, ne, 1, raw.ctypes.data, C.byref(buf)) == 0, s.error()
    s.bufs.append(buf.value)
    return buf.value


def bits(x):
    return np.ascontiguousarray(x, np.float32).ravel().view(np.uint32)


def same_values(got, want):
    """bit-equal floats, any NaN for a NaN (d = NaN times 0 is a NaN whose payload is the multiplier's business)"""
    got, want = np.ravel(got), np.ravel(want)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and same(bits(got[~nan]), bits(want[~nan]))


def quantiser_input():
    rng = np.random.default_rng(9)
    parts = [(rng.standard_normal((24, 32)) * s).astype(np.float32) for s in (1e-3, 0.05, 1.0, 40.0)] + [Q.special_blocks(), Q.tie_blocks()]
    w = np.concatenate(parts)
    assert w.shape[0] % 2 == 0
    return w.reshape(-1, 64)      # two blocks per row


def test_quantiser_matches_the_numpy_rule_bit_for_bit(sess):
    w = quantiser_input()
    rows, cols = w.shape
    d, n = Q.quantize(w)
    assert np.isnan(d).sum() == 3 and (d == 0).sum() == 1 and n.min() >= 1
    rc, q4 = new_buf(sess, sess.lib.lh_buf_quantize_q4, sess.register(w), rows, cols)
    assert rc == 0, sess.error()
    assert sess.lib.lh_buf_nfloats(sess.ctx, q4) == w.size
    got = sess.read_buf(q4, w.size)
    assert same_values(got, Q.dequantize(d, n))
    # a partial read that starts and ends inside blocks
    part = np.empty(70, np.float32)
    assert sess.lib.lh_buf_read(sess.ctx, q4, 45, part.ctypes.data_as(NP.F32P), 70) == 0, sess.error()
    assert same_values(part, Q.dequantize(d, n).ravel()[45:115])
    # the expansion holds the same values: read back (through the block-int8 reader) equal to the source read back
    rc, q8 = new_buf(sess, sess.lib.lh_buf_expand_q4, q4)
    assert rc == 0, sess.error()
    assert same_values(sess.read_buf(q8, w.size), got)
    # the same blocks registered from their 20-byte form
    reg = register_q4(sess, Q.to_blocks(d, n), rows, cols)
    assert same_values(sess.read_buf(reg, w.size), got)


def test_registered_blocks_keep_every_nibble(sess):
    rng = np.random.default_rng(10)
    rows, cols = 6, 96
    n = rng.integers(0, 16, (rows, cols // 32, 32)).astype(np.uint8)
    n[0, 0] = np.arange(32) % 16                   # all 16 nibble values in one block, n = 0 (q = -8) included
    n[1, 1] = 0
    d = (rng.standard_normal((rows, cols // 32)) * 0.02).astype(np.float32)
    d[2, 0] = -0.75
    buf = register_q4(sess, Q.to_blocks(d, n), rows, cols)
    want = Q.dequantize(d, n)
    assert want.min() < 0 and (n == 0).sum() > 32
    got = sess.read_buf(buf, rows * cols)
    assert same(bits(got), bits(want))
    rc, q8 = new_buf(sess, sess.lib.lh_buf_expand_q4, buf)
    assert rc == 0, sess.error()
    assert same(bits(sess.read_buf(q8, rows * cols)), bits(want))


def test_read_q4_returns_the_registration_blocks_and_checks_its_range(sess):
    rng = np.random.default_rng(13)
    rows, cols = 5, 64
    n = rng.integers(0, 16, (rows, cols // 32, 32)).astype(np.uint8)
    d = (rng.standard_normal((rows, cols // 32)) * 0.02).astype(np.float32)
    raw = Q.to_blocks(d, n)
    buf, nb = register_q4(sess, raw, rows, cols), rows * cols // 32
    lib = sess.lib
    out = np.zeros(nb * 20, np.uint8)
    assert lib.lh_buf_read_q4(sess.ctx, buf, 0, out.ctypes.data, nb) == 0, sess.error()
    assert out.tobytes() == raw.tobytes()
    part = np.full(3 * 20 + 4, 0xEE, np.uint8)                      # blocks [4, 7), and nothing written behind them
    assert lib.lh_buf_read_q4(sess.ctx, buf, 4, part.ctypes.data, 3) == 0, sess.error()
    assert part[:60].tobytes() == raw[80:140].tobytes() and (part[60:] == 0xEE).all()
    assert lib.lh_buf_read_q4(sess.ctx, buf, nb, out.ctypes.data, 0) == 0           # an empty range at the end
    for b0, cnt in ((0, nb + 1), (nb, 1), (nb + 1, 0), (2 ** 63, 2 ** 63)):
        assert lib.lh_buf_read_q4(sess.ctx, buf, b0, out.ctypes.data, cnt) == LH_EINVAL, (b0, cnt)
    assert lib.lh_buf_read_q4(sess.ctx, buf, 0, None, 1) == LH_EINVAL
    assert lib.lh_buf_read_q4(sess.ctx, 10 ** 9, 0, out.ctypes.data, 1) == LH_EINVAL
    rc, q8 = new_buf(sess, lib.lh_buf_expand_q4, buf)
    assert rc == 0
    f32 = sess.register(np.zeros(64, np.float32))
    for other in (q8, f32):
        assert lib.lh_buf_read_q4(sess.ctx, other, 0, out.ctypes.data, 1) == LH_EINVAL and "int4" in sess.error()
    assert lib.lh_buf_read_q4(sess.ctx, buf, 0, out.ctypes.data, nb) == 0 and out.tobytes() == raw.tobytes()


def test_refusals_name_their_reason_and_leave_the_context_usable(sess):
    lib = sess.lib
    w = (np.random.default_rng(3).standard_normal((4, 64)) * 0.1).astype(np.float32)
    f32 = sess.register(w)
    rc, q4 = new_buf(sess, lib.lh_buf_quantize_q4, f32, 4, 64)
    assert rc == 0
    rc, q8 = new_buf(sess, lib.lh_buf_quantize_q8, f32, 4, 64)
    assert rc == 0
    h, nch = C.c_uint64(), C.c_uint64()
    assert lib.lh_buf_narrow_f16(sess.ctx, f32, 4, 64, C.byref(h), C.byref(nch)) == 0
    sess.bufs.append(h.value)
    for src, word in ((h.value, "f16"), (q8, "int8"), (q4, "int4")):     # only an f32 source is quantised
        assert new_buf(sess, lib.lh_buf_quantize_q4, src, 4, 64)[0] == LH_EUNSUPPORTED
        assert word in sess.error(), sess.error()
    assert new_buf(sess, lib.lh_buf_quantize_q4, f32, 8, 32 - 1)[0] != 0                       # columns % 32
    for src in (f32, q8, h.value):
        assert new_buf(sess, lib.lh_buf_expand_q4, src)[0] == LH_EINVAL
    out = np.zeros(4, np.float32)
    assert lib.lh_buf_upload(sess.ctx, q4, 0, out.ctypes.data_as(NP.F32P), 4) == LH_EINVAL and "int4" in sess.error()
    assert lib.lh_buf_fill_synth(sess.ctx, q4, 0, 64, 1, 1, 1.0, 0.0) == LH_EINVAL and "int4" in sess.error()
    assert new_buf(sess, lib.lh_buf_quantize_q8, q4, 4, 64)[0] == LH_EUNSUPPORTED and "int4" in sess.error()
    d, n = Q.quantize(w)
    assert same_values(sess.read_buf(q4, w.size), Q.dequantize(d, n))


# ---- 2. Step and Rows, byte-equal to B ---------------------------------------------------------------------------------------------------------------
# shape -> (layers, route of B's Eval of n = 2, 3..4, 5 rows as a WHOLE model on 256 CUs: eval_route / rows_path_ok / q8b_shape_ok of csrc/plan.hip).
#   "Rows"     B rides the int8 decode stream (k_gemv_q8_rows): A must show k_gemv_q4_rows and no expansion
#   "Steps"    B has neither an n-row launch nor a k_stream_q8b launch and runs n single steps (Q8Steps): A runs them on the nibbles - k_gemv_q4s only,
#              no expansion either (the plan's routes: Step, Rows and Q8Steps stay on the nibbles)
#   "Expand"   B runs k_stream_q8b over its int8 planes: A expands and runs the same launches
# odd640m32: its odd vocabulary has no two-row lm_head, F = 1728 is no multiple of 128.  13Blayer (K16 = 320 and 864) and 65Blayer (K16 = 512 and 1376)
# have no n-row instantiation; the 13B layer has k_stream_q8b launches from three rows on, the 65B layer's w1|w3 has none.
STEP_SHAPES = {
    "small": (2, "Rows", "Rows", "Expand"),
    "odd640m32": (2, "Steps", "Steps", "Steps"),
    "7Blayer": (2, "Rows", "Rows", "Expand"),
    "13Blayer": (1, "Steps", "Expand", "Expand"),
    "65Blayer": (1, "Steps", "Steps", "Steps"),
}
STEP_CTX = 64
SHAPE_KW = dict(WP.SHAPES, **{"13Blayer": dict(vocab=2048, embd=5120, mult=256, heads=40)})


@pytest.mark.parametrize("shape", list(STEP_SHAPES))
def test_step_and_rows_are_byte_equal_to_the_expanded_model(product, shape):
    layers, r2, r34, r5 = STEP_SHAPES[shape]
    hp = make_hparams(**SHAPE_KW[shape], layers=layers, ctx=STEP_CTX)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(STEP_CTX, 1), B.NewContext(STEP_CTX, 1)
    seeded_cache((ca, cb), hp, layers, STEP_CTX)
    rng = np.random.default_rng(11)
    seen_step = False
    try:
        for past in (0, 37):
            for n in (1, 2, 3, 4, 5):
                toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
                la, tr = route_trace(lambda: poisoned(ca).Eval(toks, past))
                assert fused(product, ca) == 1
                lb = cb.Eval(toks, past)
                assert np.isfinite(lb).all() and np.abs(lb).max() > 0
                assert same(la, lb), (shape, n, past, float(np.abs(la - lb).max()))
                names = set(families(tr))
                route = "Step" if n == 1 else r2 if n == 2 else r34 if n <= 4 else r5
                # (a launch replayed from the captured one-token graph records nothing: the step's kernels show at its first Eval)
                if route == "Step":
                    assert not names & {"k_gemv_q4_rows", "k_expand_q4"}, tr
                    assert seen_step or "k_gemv_q4s" in names, tr
                    seen_step = True
                elif route == "Rows":
                    assert "k_gemv_q4_rows" in names and "k_expand_q4" not in names, tr
                elif route == "Steps":
                    assert "k_gemv_q4s" in names and not names & {"k_gemv_q4_rows", "k_expand_q4"}, tr
                else:
                    assert "k_expand_q4" in names and "k_gemv_q4_rows" not in names, tr
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 3. the expanded route ---------------------------------------------------------------------------------------------------------------------------
def test_expanded_route_runs_the_int8_schedule_byte_equal(product):
    ctx = 192
    hp = make_hparams(**WP.SHAPES["7Blayer"], layers=2, ctx=ctx)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    seeded_cache((ca, cb), hp, 2, ctx)
    rng = np.random.default_rng(12)
    try:
        cases = [(n, past) for past in (0, 37) for n in (5, 9, 64, 89, 130)] + [(5, 0)]       # (5 again behind 130: the image does not move)
        for n, past in cases:
            toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
            assert fused(product, ca) == 1
            lb, tb = route_trace(lambda: cb.Eval(toks, past))
            assert same(la, lb), (n, past, float(np.abs(la - lb).max()))
            fa = families(ta)
            assert fa[0] == "k_expand_q4" and fa.count("k_expand_q4") >= 14, ta        # seven matrices per layer, in front of the layer's launches
            assert "k_gemv_q4_rows" not in fa
            assert not set(families(tb)) & set(Q4_KERNELS), tb
            assert [e for e in ta if e.split("<")[0] not in Q4_KERNELS] == tb, (n, past)   # B's kernels in B's order
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 4. loops and batches ----------------------------------------------------------------------------------------------------------------------------
SMALL_PROMPT = [t % SHAPES["small"]["vocab"] for t in PROMPT]     # the benchmark's 8-token prompt inside the small vocabulary


@pytest.fixture(scope="module")
def small_twins(product):
    hp = make_hparams(**SHAPES["small"], ctx=64)
    A, B = twins(product, hp, seed=1234)
    yield hp, A, B
    A.free(); B.free()


def on_both(small_twins, fn):
    hp, A, B = small_twins
    res = []
    for m in (A, B):
        c = m.NewContext(64, 1)
        try:
            res.append(fn(c))
        finally:
            c.free()
    return res


def test_greedy_loops_and_the_contract_route(product, small_twins):
    def run(c):
        ids, lg = c.GreedyDecode(SMALL_PROMPT, 24)
        more = c.GreedyContinue(ids[-1], len(SMALL_PROMPT) + 23, 8)      # the contract route: one llama_Eval = one lh_graph_compute per token
        assert fused(product, c) == 1
        return ids, lg, more
    (ia, la, ma), (ib, lb, mb) = on_both(small_twins, run)
    assert ia == ib and ma == mb and same(la, lb)
    assert len(set(ia)) > 4


def test_contract_route_per_token_is_fused_and_equal(product, small_twins):
    def run(c):
        out = [c.Eval(SMALL_PROMPT, 0)]
        for i in range(6):
            out.append(c.Eval([int(np.argmax(out[-1]))], len(SMALL_PROMPT) + i))
            assert fused(product, c) == 1
        return np.stack(out)
    a, b = on_both(small_twins, run)
    assert same(a, b)


def test_sampled_loop(small_twins):
    a, b = on_both(small_twins, lambda c: c.SampleDecode(SMALL_PROMPT, 24, topK=40, seed=3))
    assert a == b


def test_lookup_loop(small_twins):
    def run(c):
        first = int(np.argmax(c.Eval(SMALL_PROMPT, 0)))
        return c.DecodeLookup(first, len(SMALL_PROMPT), 24, 3, want_logits=True)
    (ia, la, sa, ta), (ib, lb, sb, tb) = on_both(small_twins, run)
    assert ia == ib and same(la, lb) and sa == sb and ta == tb


def test_score(small_twins):
    toks = [int(t) for t in np.random.default_rng(3).integers(0, SHAPES["small"]["vocab"], 16)]
    a, b = on_both(small_twins, lambda c: c.Score(toks, 0))
    assert same(a, b)


@pytest.mark.parametrize("pods", [2, 4, 5])
def test_batch_ticks(small_twins, pods):
    hp, A, B = small_twins
    rng = np.random.default_rng(40 + pods)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 3 + i % 4)] for i in range(pods)]
    res = []
    for m in (A, B):
        b = Batch(m, 64, pods)
        try:
            assert b.batched, "these shapes must take the one-pass route"
            res.append(poisoned(b, m is A).GreedyDecode(prompts, 6, want_logits=True))
        finally:
            b.free()
    (ia, la), (ib, lb) = res
    assert ia == ib and same(la, lb)
    if pods <= 4:   # the Rows bit-identity: a pod decodes the same bytes alone (k_gemv_q4s) and in a tick of 2..4 (k_gemv_q4_rows)
        for i in range(pods):
            c = A.NewContext(64, 1)
            ids, lg = c.GreedyDecode(prompts[i], 6)
            c.free()
            assert ids == ia[i] and same(lg[-1], la[i]), i


def test_batch_feed(small_twins):
    hp, A, B = small_twins
    rng = np.random.default_rng(50)
    toks = [[int(t) for t in rng.integers(0, hp.vocabSize, 5)] for _ in range(3)]
    res = []
    for m in (A, B):
        b = Batch(m, 64, 3)
        try:
            res.append(poisoned(b, m is A).Feed(toks, [0, 0, 0], want_logits=True, want_rows=True))
        finally:
            b.free()
    (ia, la, ra), (ib, lb, rb) = res
    assert ia == ib and same(la, lb) and same(ra, rb)


def test_batch_fork_with_a_shared_prefix(small_twins):
    hp, A, B = small_twins
    rng = np.random.default_rng(51)
    prefix = [int(t) for t in rng.integers(0, hp.vocabSize, 12)]
    sfx = [[int(t) for t in rng.integers(0, hp.vocabSize, 2 + i)] for i in range(3)]
    res = []
    for m in (A, B):
        b = Batch(m, 64, 3)
        try:
            poisoned(b, m is A).Feed([prefix, [1], [2]], [0, 0, 0])
            b.Fork(0, [1, 2], len(prefix))
            pending = poisoned(b, m is A).Feed(sfx, [len(prefix)] * 3)
            pos = [len(prefix) + len(s) for s in sfx]
            res.append((pending, b.ShareInfo()) + tuple(poisoned(b, m is A).Decode(pending, pos, 8, want_logits=True)))
        finally:
            b.free()
    (pa, sa, ia, la), (pb, sb, ib, lb) = res
    assert pa == pb and sa == sb and ia == ib and same(la, lb)


def test_q4_twin_drafts_for_its_fp32_target(product, small_twins):
    """lossless draft-model decoding: an fp32 target with its own block-int4 form as the draft gives the target's greedy ids and last logits"""
    hp, A, B = small_twins
    T = product.NewSyntheticModel(hp, 1234)
    N = 20
    lone = T.NewContext(64, 1)
    pair = DraftPair(T, A, 64)
    try:
        first = int(np.argmax(lone.Eval(SMALL_PROMPT, 0)))
        want_ids, want_lg = decode_greedy_resident(lone, first, len(SMALL_PROMPT), N, want_logits=True)
        assert int(np.argmax(pair.target.Eval(SMALL_PROMPT, 0))) == first
        pair.draft.Eval(SMALL_PROMPT, 0)
        ids, lg, st, tr = pair.DecodeDraft(first, len(SMALL_PROMPT), N, 3, want_logits=True)
        assert ids == want_ids and same(lg, want_lg)
        assert st["drafted"] > 0
    finally:
        pair.free(); lone.free(); T.free()


# ---- 5. refusals at the model level ------------------------------------------------------------------------------------------------------------------
def test_model_level_refusals_leave_everything_usable(product, small_twins):
    hp, A, B = small_twins
    with pytest.raises(MLError, match="int4"):
        A.QuantizeQ8()
    with pytest.raises(MLError, match="int4"):
        A.NarrowF16()
    with pytest.raises(MLError, match="int4"):
        A.SetTensor("output.weight", np.zeros((hp.vocabSize, hp.embdSize), np.float32))
    with pytest.raises(MLError):
        A.Save(os.devnull, 1)
    assert "int4" in product.last_error()
    with pytest.raises(MLError, match="int4"):
        B.ExpandQ4()                                   # a block-int8 model is not expanded again
    c = A.NewContext(64, 1)
    try:
        before = c.Eval(SMALL_PROMPT, 0)
        with pytest.raises(MLError, match="alive"):
            A.ExpandQ4()
        with pytest.raises(MLError, match="alive"):
            m = product.NewSyntheticModel(make_hparams(**SHAPES["tiny"], ctx=16), 3)
            c2 = m.NewContext(16, 1)
            try:
                m.QuantizeQ4()
            finally:
                c2.free(); m.free()
        assert A.weight_type == 2
        os.environ["LLAMAGO_NO_FUSION"] = "1"
        try:
            with pytest.raises(MLError, match="int4"):
                c.Eval(SMALL_PROMPT, 0)
        finally:
            del os.environ["LLAMAGO_NO_FUSION"]
        assert same(c.Eval(SMALL_PROMPT, 0), before)
        assert fused(product, c) == 1
    finally:
        c.free()


# ---- 6. files ----------------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILE_SMALL_PROMPT = [1, 70, 261, 5, 280, 33, 9]      # tests/test_gpu_llama.py: the golden prompt of the reference converter's files


def parse_ggjt(path):
    """(hyper-parameters, {tensor name: (dtype, ne, raw bytes)} in file order, the bytes in front of the first tensor) of a ggjt file (magic, version,
    7 hyper-parameters, vocabulary, tensors aligned to 32 bytes)"""
    raw = open(path, "rb").read()
    u32 = lambda o: int.from_bytes(raw[o:o + 4], "little")      # noqa: E731
    assert u32(0) == 0x67676a74 and u32(4) == 1
    hp = [u32(8 + 4 * i) for i in range(7)]
    o = 36
    for _ in range(hp[0]):
        o += 4 + u32(o) + 4
    out, head = {}, raw[:o]
    while o + 12 <= len(raw):
        dims, nlen, dtype = u32(o), u32(o + 4), u32(o + 8)
        ne = [u32(o + 12 + 4 * i) for i in range(dims)]
        o += 12 + 4 * dims
        name = raw[o:o + nlen].decode()
        o = (o + nlen + 31) & ~31
        n = int(np.prod(ne))
        size = {0: n * 4, 1: n * 2, 2: n // 32 * 20}[dtype]
        out[name] = (dtype, ne, raw[o:o + size])
        o += size
    return hp, out, head


def write_ggjt(path, head, tensors):
    """the inverse of parse_ggjt"""
    with open(path, "wb") as f:
        f.write(head)
        for name, (dtype, ne, data) in tensors.items():
            f.write(b"".join(int(v).to_bytes(4, "little") for v in [len(ne), len(name.encode()), dtype] + list(ne)))
            f.write(name.encode())
            f.write(b"\0" * (-f.tell() % 32))
            f.write(bytes(data))


def test_saved_q4_file_loads_back_block_for_block(product, tmp_path):
    hp = make_hparams(**SHAPES["tiny"], ctx=32)
    F = product.NewSyntheticModel(hp, 21)
    wq = np.array(product.read(None, F.tensor("layers.1.attention.wq.weight")), np.float32).reshape(hp.embdSize, hp.embdSize)
    F.free()
    A = product.NewSyntheticModel(hp, 21).QuantizeQ4()
    path = str(tmp_path / "tiny_q4.bin")
    A.SaveQ4(path)
    header, tensors, head = parse_ggjt(path)
    again = str(tmp_path / "again.bin")
    write_ggjt(again, head, tensors)
    assert open(again, "rb").read() == open(path, "rb").read()          # (the writer of the mixed-file test below reproduces the file)
    assert header[6] == 2 and len(tensors) == 3 + 9 * hp.layersCount
    assert all(t[0] == (2 if (n.endswith("weight") and len(t[1]) == 2 and n != "tok_embeddings.weight") else 0) for n, t in tensors.items())
    dtype, ne, raw = tensors["layers.1.attention.wq.weight"]
    d, n = Q.quantize(wq)
    assert ne == [hp.embdSize, hp.embdSize] and bytes(raw) == Q.to_blocks(d, n).tobytes()      # the device quantiser = the numpy rule, in the file's layout
    K = product.LoadModelKeepQ4(path, 32)
    assert K.weight_type == 2
    with pytest.raises(MLError):
        product.LoadModel(path, 32)                     # llama_LoadModel's own refusal stays
    ca, ck = A.NewContext(32, 1), K.NewContext(32, 1)
    try:
        for toks, past in ((FILE_SMALL_PROMPT, 0), ([5], 7), ([9, 8, 7], 8), (list(range(1, 14)), 11)):
            assert same(poisoned(ca).Eval(toks, past), ck.Eval(toks, past)), (toks, past)
    finally:
        ca.free(); ck.free(); A.free(); K.free()


@pytest.mark.parametrize("name", ["ref_ggjt_f16_2parts.bin", "ref_ggjt_f32.bin"])
def test_files_without_q4_matrices_load_as_ever(product, name):
    path = os.path.join(GOLDEN, name)
    mk, mw = product.LoadModelKeepQ4(path, 32), product.LoadModel(path, 32)
    assert mk.weight_type == 0
    ck, cw = mk.NewContext(32, 1), mw.NewContext(32, 1)
    try:
        assert same(ck.Eval(FILE_SMALL_PROMPT, 0), cw.Eval(FILE_SMALL_PROMPT, 0))
    finally:
        ck.free(); cw.free(); mk.free(); mw.free()


def refusal(fn):
    """the message a load is refused with"""
    with pytest.raises(MLError) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("case", ["one_f16_matrix", "output_f16", "one_matrix_missing"])
def test_q4_file_with_a_matrix_that_is_not_q4_loads_as_llama_loadmodel_loads_it(product, tmp_path, case):
    """The input on which LoadModelKeepQ4's look over the tensor headers decides something: a Q4_0 file in which ONE of the 7 L + 1 matrices is f16 (the
    first matrix of a layer in the middle of the file, or the output matrix), or is not there at all.  The file must load exactly as llama_LoadModel
    loads it - which, the other matrices being Q4_0, is llama_LoadModel's own refusal - and leave nothing behind: the next load of the whole file works."""
    hp = make_hparams(**SHAPES["tiny"], ctx=32)
    A = product.NewSyntheticModel(hp, 21).QuantizeQ4()
    good = str(tmp_path / "tiny_q4.bin")
    A.SaveQ4(good)
    _, tensors, head = parse_ggjt(good)
    victim = "output.weight" if case == "output_f16" else "layers.1.feed_forward.w1.weight"
    dtype, ne, raw = tensors[victim]
    assert dtype == 2
    if case == "one_matrix_missing":
        del tensors[victim]
    else:
        d, n = Q.from_blocks(np.frombuffer(raw, np.uint8), ne[1], ne[0])
        tensors[victim] = (1, ne, Q.dequantize(d, n).astype(np.float16).tobytes())
    mixed = str(tmp_path / "mixed.bin")
    write_ggjt(mixed, head, tensors)
    assert len(parse_ggjt(mixed)[1]) == 3 + 9 * hp.layersCount - (case == "one_matrix_missing")
    plain = refusal(lambda: product.LoadModel(mixed, 32))
    kept = refusal(lambda: product.LoadModelKeepQ4(mixed, 32))
    assert kept.replace("llamago_LoadModelKeepQ4", "llama_LoadModel") == plain and "not supported" in plain, (kept, plain)
    K = product.LoadModelKeepQ4(good, 32)                      # nothing half-registered stands in the way of the whole file
    assert K.weight_type == 2
    ca, ck = A.NewContext(32, 1), K.NewContext(32, 1)
    try:
        assert same(poisoned(ca).Eval(FILE_SMALL_PROMPT, 0), ck.Eval(FILE_SMALL_PROMPT, 0))
    finally:
        ca.free(); ck.free(); A.free(); K.free()
