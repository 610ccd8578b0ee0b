"""gpu: f16 weight matrices kept f16 in HBM (dtype 1; csrc/kernels_f16.h) - every comparison is == on bytes or ids, no tolerance anywhere
but the one inherited number of the file test.

The reference of every model test is the same.  Model A is a synthetic model narrowed with NarrowF16; model B is the same seed narrowed and then widened
with WidenF16: an fp32 model, which runs only the fp32 kernels the rest of the suite holds to the checker.  A and B hold the same values, and widening is
exact, so whatever A computes has to be B's bytes: on the f16 forms of the decode stream (one row, 2..8 rows), which keep the fp32 kernels' lane -> column
map and summation order, and on every other route, where A runs B's kernels over an fp32 image."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import node_path_abi as NP            # noqa: E402
import weight_probe_ref as WP         # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, MLError, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LH_EINVAL, LH_EUNSUPPORTED = -1, -4
F16_KERNELS = ("k_gemv_sa_h", "k_gemv_rows_h", "k_widen_f16")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def families(trace):
    """kernel names of a route trace without template arguments and suffixes: 'k_gemv_sa_h<4,4,256>' -> 'k_gemv_sa_h'"""
    return [e.split("<")[0].split("/")[0] for e in trace]


def fused(product, c):
    product.lib.llamago_LastGraphFused.restype = C.c_int
    product.lib.llamago_LastGraphFused.argtypes = [C.c_void_p]
    product.lib.llama_MLContext.restype = C.c_void_p
    return product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h))


def twins(product, hp, seed=77, prepare=None):
    """(A, B): the same synthetic values as f16 and as fp32; prepare(model) runs on both while they hold f16-exact fp32 values"""
    out = []
    for widen in (False, True):
        m = product.NewSyntheticModel(hp, seed)
        assert m.weight_type == 0
        assert m.NarrowF16() > 0                    # synthetic fp32 weights are not halves
        if prepare is not None:                     # f16-exact values first, so that the second narrowing changes nothing
            m.WidenF16()
            prepare(m)
            assert m.NarrowF16() == 0
        assert m.weight_type == 1
        if widen:
            m.WidenF16()
            assert m.weight_type == 0
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


# ---- 1. conversions, op level ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip(product):
    import llama_go_amd as pkg
    lib = NP.bind(C.CDLL(pkg.LIBLLAMAHIP))
    lib.lh_buf_narrow_f16.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.lh_buf_widen_f16.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.lh_buf_upload.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, NP.F32P, C.c_uint64]
    lib.lh_buf_quantize_q8.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.lh_buf_nfloats.restype = C.c_uint64
    lib.lh_buf_nfloats.argtypes = [C.c_void_p, C.c_uint64]
    return lib


@pytest.fixture()
def sess(hip):
    s = NP.Session(hip)
    yield s
    s.close()


def register_f16(s, halves, rows, cols):
    halves = np.ascontiguousarray(halves, dtype=np.uint16)
    ne = (C.c_uint32 * 4)(cols, rows, 1, 1)
    buf = C.c_uint64()
    assert s.lib.lh_tensor_register(s.ctx, 0, 1, ne, 1, halves.ctypes.data, C.byref(buf)) == 0, s.error()
    s.bufs.append(buf.value)
    return buf.value


def widen(s, buf):
    out = C.c_uint64()
    assert s.lib.lh_buf_widen_f16(s.ctx, buf, C.byref(out)) == 0, s.error()
    s.bufs.append(out.value)
    return out.value


def narrow(s, buf, rows, cols):
    out, n = C.c_uint64(), C.c_uint64(12345)
    assert s.lib.lh_buf_narrow_f16(s.ctx, buf, rows, cols, C.byref(out), C.byref(n)) == 0, s.error()
    s.bufs.append(out.value)
    return out.value, int(n.value)


ALL_HALVES = np.arange(65536, dtype=np.uint16)
NOT_NAN = ~np.isnan(ALL_HALVES.view(np.float16))


def test_widen_is_exact_on_every_half_pattern(sess):
    assert int(NOT_NAN.sum()) == 63490
    h = register_f16(sess, ALL_HALVES, 256, 256)
    assert sess.lib.lh_buf_nfloats(sess.ctx, h) == 65536
    got = sess.read_buf(widen(sess, h), 65536)
    want = ALL_HALVES.view(np.float16).astype(np.float32)
    assert same(got.view(np.uint32)[NOT_NAN], want.view(np.uint32)[NOT_NAN])      # both zeros, the 2046 subnormals, +-65504, +-inf among them
    assert np.isnan(got[~NOT_NAN]).all() and int((~NOT_NAN).sum()) == 2046
    # an f16 buffer holds no floats: upload and read are refused, and the context goes on working
    out = np.empty(4, np.float32)
    assert sess.lib.lh_buf_read(sess.ctx, h, 0, out.ctypes.data_as(NP.F32P), 4) == LH_EINVAL
    assert sess.lib.lh_buf_upload(sess.ctx, h, 0, out.ctypes.data_as(NP.F32P), 4) == LH_EINVAL
    q = C.c_uint64()
    assert sess.lib.lh_buf_quantize_q8(sess.ctx, h, 256, 256, C.byref(q)) == LH_EUNSUPPORTED
    assert same(sess.read_buf(widen(sess, h), 65536).view(np.uint32)[NOT_NAN], want.view(np.uint32)[NOT_NAN])


def narrow_fixture():
    """fp32 values around every rounding decision of f32 -> f16: ties with an even and an odd lower neighbour (normal and subnormal results), values
    just beside the ties, values that land subnormal or flush to zero, the largest value below the overflow threshold, the threshold, overflow, -0"""
    f = np.float32
    v = []
    for lo in (0x3C00, 0x3C01, 0x0400, 0x0401, 0x0001, 0x0002, 0x03FF, 0x7BFE, 0x7BFF, 0x0000):   # a half and the next one up
        a, b = np.array([lo, lo + 1], np.uint16).view(np.float16).astype(np.float64)
        mid = f((a + b) / 2) if np.isfinite(b) else f(65520.0)
        v += [f(a), mid, np.nextafter(mid, f(0)), np.nextafter(mid, f(np.inf))]
    v += [f(2.0 ** -24), f(2.0 ** -25), np.nextafter(f(2.0 ** -25), f(1)), f(2.0 ** -26), f(6.1e-5), f(1e-7), f(3e-8), f(1e-10), f(1e-40)]
    v += [np.nextafter(f(65520.0), f(0)), f(65520.0), f(65536.0), f(1e6), f(3.4e38), f(np.inf), f(65504.0), f(0.0), f(1.0), f(0.1), f(1 / 3)]
    v = np.array(v, dtype=np.float32)
    v = np.concatenate([v, -v])          # -0 among them
    return np.concatenate([v, np.zeros((-len(v)) % 4 + 3, np.float32)])   # a length that is no multiple of four: the kernel's scalar tail


def test_narrow_rounds_as_numpy_does(sess):
    x = narrow_fixture()
    assert x.size % 4 == 3
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    changed = int((want.astype(np.float32) != x).sum())
    assert changed > 40
    h, n = narrow(sess, sess.register(x), 1, x.size)
    assert n == changed
    got = sess.read_buf(widen(sess, h), x.size)
    assert same(got.view(np.uint32), want.astype(np.float32).view(np.uint32))   # widening is exact (test above): equal floats <=> equal halves, -0 kept
    assert np.signbit(got[np.flatnonzero((x == 0) & np.signbit(x))]).all()


def test_narrow_after_widen_is_the_identity(sess):
    f32 = widen(sess, register_f16(sess, ALL_HALVES, 256, 256))
    h, n = narrow(sess, f32, 256, 256)
    assert n == 0
    got = sess.read_buf(widen(sess, h), 65536)
    want = ALL_HALVES.view(np.float16).astype(np.float32)
    assert same(got.view(np.uint32)[NOT_NAN], want.view(np.uint32)[NOT_NAN])
    assert np.isnan(got[~NOT_NAN]).all()


# ---- 2. Step and Rows, byte-equal to B --------------------------------------------------------------------------------------------------------------
# shape -> (layers, rows the decode stream carries for the WHOLE model of that shape, f16 as fp32: rows_path_ok of csrc/plan.hip).  The odd vocabulary of
# odd640 has no two-row lm_head and 65Blayer's K = 22016 no n-row instantiation, so their Evals of 2..8 rows take the route an fp32 model of the shape
# takes - the widened one - and only their one-row Evals run an f16 kernel (odd640: inactive lanes; 65Blayer: the 512- and 1024-thread forms);
# odd640v516 is odd640 with an even vocabulary, so that the inactive lanes and the odd head count also go through k_gemv_rows_h.
STEP_SHAPES = {"small": (2, 8), "odd640": (2, 1), "odd640v516": (2, 8), "7Blayer": (2, 8), "65Blayer": (1, 1)}
STEP_CTX = 64
SHAPE_KW = dict(WP.SHAPES, odd640v516=dict(WP.SHAPES["odd640"], vocab=516))


@pytest.mark.parametrize("shape", list(STEP_SHAPES))
def test_step_and_rows_are_byte_equal_to_the_widened_model(product, shape):
    layers, rows_max = STEP_SHAPES[shape]
    hp = make_hparams(**SHAPE_KW[shape], layers=layers, ctx=STEP_CTX)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(STEP_CTX, 1), B.NewContext(STEP_CTX, 1)
    seeded_cache((ca, cb), hp, layers, STEP_CTX)
    rng = np.random.default_rng(11)
    seen_step = False
    try:
        for past in (0, 37):
            for n in (1, 2, 3, 4, 5, 8):
                toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
                la, tr = route_trace(lambda: poisoned(ca).Eval(toks, past))
                assert fused(product, ca) == 1
                lb = cb.Eval(toks, past)
                assert np.isfinite(lb).all() and np.abs(lb).max() > 0
                assert same(la, lb), (shape, n, past, float(np.abs(la - lb).max()))
                names = set(families(tr))
                assert not names & {"k_gemv_sa", "k_gemv_rows"}, tr
                # (a launch replayed from the captured one-token graph records nothing: the step's kernels show at its first Eval)
                if n == 1:
                    assert not names & {"k_gemv_rows_h", "k_widen_f16"}, tr
                    assert seen_step or "k_gemv_sa_h" in names, tr
                    seen_step = True
                elif n <= rows_max:
                    assert "k_gemv_rows_h" in names and "k_widen_f16" not in names, tr
                else:
                    assert "k_widen_f16" in names and "k_gemv_rows_h" not in names, tr
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 3. subnormal weights inside the GEMV ------------------------------------------------------------------------------------------------------------
def test_subnormal_output_weights_reach_the_logits(product):
    kw = WP.SHAPES["small"]
    hp = make_hparams(**kw, layers=2, ctx=STEP_CTX)
    V, d = kw["vocab"], kw["embd"]
    pat = np.arange(V * d, dtype=np.int64) % 1100 + 1          # half patterns 0x0001 .. 0x044C: all 1023 subnormals and the smallest normals
    halves = pat.astype(np.uint16) | ((np.arange(V * d) & 1).astype(np.uint16) << 15)   # alternating sign
    out = halves.view(np.float16).astype(np.float32).reshape(V, d)
    assert int((np.abs(out) < 2.0 ** -14).sum()) > V * d // 2 and (out != 0).all()
    A, B = twins(product, hp, prepare=lambda m: m.SetTensor("output.weight", out))
    ca, cb = A.NewContext(STEP_CTX, 1), B.NewContext(STEP_CTX, 1)
    try:
        for toks in ([7], [3, 99, 1024, 5]):
            la, lb = poisoned(ca).Eval(toks, 0), cb.Eval(toks, 0)
            assert same(la, lb)
            assert np.count_nonzero(la) > V // 2          # a conversion that flushed subnormals would leave (mostly) zeros
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 4. the widened route ------------------------------------------------------------------------------------------------------------------------------
def test_widened_route_runs_the_fp32_schedule_byte_equal(product):
    ctx = 192
    hp = make_hparams(**WP.SHAPES["7Blayer"], layers=2, ctx=ctx)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    seeded_cache((ca, cb), hp, 2, ctx)
    rng = np.random.default_rng(12)
    try:
        for n, past in ((9, 0), (17, 0), (64, 0), (130, 0), (9, 37), (17, 37), (64, 37), (130, 37), (9, 0)):   # (9 again behind 130: the image does not move)
            toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
            assert fused(product, ca) == 1
            lb, tb = route_trace(lambda: cb.Eval(toks, past))
            assert same(la, lb), (n, past, float(np.abs(la - lb).max()))
            fa = families(ta)
            assert fa[0] == "k_widen_f16" and fa.count("k_widen_f16") >= 14, ta        # seven matrices per layer, in front of the layer's launches
            assert "k_gemv_rows_h" not in fa
            assert not set(families(tb)) & set(F16_KERNELS), tb
            assert [e for e in ta if e.split("<")[0] not in F16_KERNELS] == tb, (n, past)   # B's kernels in B's order
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 5. loops and batches ----------------------------------------------------------------------------------------------------------------------------
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


def test_greedy_loops(product, small_twins):
    def run(c):
        ids, lg = c.GreedyDecode(SMALL_PROMPT, 24)
        more = c.GreedyContinue(ids[-1], len(SMALL_PROMPT) + 23, 8)      # the contract route: one lh_graph_compute per token
        assert fused(product, c) == 1
        return ids, lg, more
    (ia, la, ma), (ib, lb, mb) = on_both(small_twins, run)
    assert ia == ib and ma == mb and same(la, lb)
    assert len(set(ia)) > 4


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


@pytest.mark.parametrize("pods", [2, 8, 9])
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
    if pods <= 8:   # the Rows bit-identity: a pod decodes the same bytes alone (k_gemv_sa_h) and in a tick of 2..8 (k_gemv_rows_h)
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


# ---- 6. files ----------------------------------------------------------------------------------------------------------------------------------------
FILE_SMALL_PROMPT = [1, 70, 261, 5, 280, 33, 9]      # tests/test_gpu_llama.py: the golden prompt of the reference converter's files


def test_f16_file_keeps_its_halves(product, oracle):
    from test_gpu_llama import TOL, rel            # the inherited tolerance of product logits against the checker's
    path = os.path.join(GOLDEN, "ref_ggjt_f16_2parts.bin")
    mk, mw, mo = product.LoadModelKeepF16(path, 32), product.LoadModel(path, 32), oracle.LoadModel(path, 32)
    assert mk.weight_type == 1 and mw.weight_type == 0
    ck, cw, co = mk.NewContext(32, 1), mw.NewContext(32, 1), mo.NewContext(32, 2, False)
    try:
        assert same(ck.Eval(FILE_SMALL_PROMPT, 0), cw.Eval(FILE_SMALL_PROMPT, 0))
        ik, lk = ck.GreedyDecode(FILE_SMALL_PROMPT, 6)
        iw, lw = cw.GreedyDecode(FILE_SMALL_PROMPT, 6)
        io, lo = co.GreedyDecode(FILE_SMALL_PROMPT, 6)
        assert ik == iw and same(lk, lw)
        assert ik == io and rel(lk, lo) <= TOL
    finally:
        ck.free(); cw.free(); co.free(); mk.free(); mw.free(); mo.free()


def test_f32_file_loads_as_ever(product):
    path = os.path.join(GOLDEN, "ref_ggjt_f32.bin")
    mk, mw = product.LoadModelKeepF16(path, 32), product.LoadModel(path, 32)
    assert mk.weight_type == 0
    ck, cw = mk.NewContext(32, 1), mw.NewContext(32, 1)
    try:
        assert same(ck.Eval(FILE_SMALL_PROMPT, 0), cw.Eval(FILE_SMALL_PROMPT, 0))
    finally:
        ck.free(); cw.free(); mk.free(); mw.free()


# ---- 7. refusals, context left usable ----------------------------------------------------------------------------------------------------------------
class LlamaLayer(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("attention_norm", "wq", "wk", "wv", "wo", "ffn_norm", "w1", "w2", "w3")]


class LlamaDesc(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("vocab", "embd", "heads", "layers", "ff", "ctx", "layer0", "layer1")] + \
               [(k, C.c_uint64) for k in ("tok_embeddings", "norm", "output")] + [("layer", C.POINTER(LlamaLayer)), ("k_cache", C.c_uint64), ("v_cache", C.c_uint64),
                                                                                   ("weight_dtype", C.c_int)]


def test_llama_create_refuses_an_f32_matrix_in_an_f16_model(sess):
    V, d, H, F, ctx = 64, 128, 2, 256, 16
    lib = sess.lib
    lib.lh_llama_create.argtypes = [C.c_void_p, C.POINTER(LlamaDesc), C.POINTER(C.c_void_p)]
    lib.lh_llama_destroy.argtypes = [C.c_void_p]
    lib.lh_llama_eval.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, NP.F32P]
    rng = np.random.default_rng(1)
    f32 = lambda *s: sess.register((rng.standard_normal(s) * 0.05).astype(np.float32))             # noqa: E731
    f16 = lambda r, c: register_f16(sess, (rng.standard_normal((r, c)) * 0.05).astype(np.float16).view(np.uint16), r, c)   # noqa: E731
    lay = LlamaLayer(f32(d) , f16(d, d), f16(d, d), f16(d, d), f16(d, d), f32(d), f16(F, d), f16(d, F), f16(F, d))
    desc = LlamaDesc(V, d, H, 1, F, ctx, 0, 1, f32(V, d), f32(d), f16(V, d), C.pointer(lay), f32(ctx * d), f32(ctx * d), 1)
    out = C.c_void_p()
    good_wo = lay.wo
    lay.wo = f32(d, d)
    assert lib.lh_llama_create(sess.ctx, C.byref(desc), C.byref(out)) == LH_EINVAL and not out.value
    assert "f16" in sess.error()
    lay.wo = good_wo                                  # the context is as usable as before: the all-f16 description is accepted and evaluates
    assert lib.lh_llama_create(sess.ctx, C.byref(desc), C.byref(out)) == 0, sess.error()
    toks = (C.c_uint32 * 3)(1, 2, 3)
    lg = np.empty(V, np.float32)
    assert lib.lh_llama_eval(out, toks, 3, 0, lg.ctypes.data_as(NP.F32P)) == 0, sess.error()
    assert np.isfinite(lg).all() and np.abs(lg).max() > 0
    lib.lh_llama_destroy(out)


def test_model_level_refusals_leave_everything_usable(product, small_twins):
    hp, A, B = small_twins
    with pytest.raises(MLError, match="f16"):
        A.QuantizeQ8()
    with pytest.raises(MLError, match="f16"):
        A.SetTensor("output.weight", np.zeros((hp.vocabSize, hp.embdSize), np.float32))
    c = A.NewContext(64, 1)
    try:
        before = c.Eval(SMALL_PROMPT, 0)
        with pytest.raises(MLError, match="alive"):
            m = product.NewSyntheticModel(make_hparams(**SHAPES["tiny"], ctx=16), 3)
            c2 = m.NewContext(16, 1)
            try:
                m.NarrowF16()
            finally:
                c2.free(); m.free()
        with pytest.raises(MLError):
            A.Save(os.devnull, 1)
        assert A.weight_type == 1
        os.environ["LLAMAGO_NO_FUSION"] = "1"
        try:
            with pytest.raises(MLError, match="f16"):
                c.Eval(SMALL_PROMPT, 0)
        finally:
            del os.environ["LLAMAGO_NO_FUSION"]
        assert same(c.Eval(SMALL_PROMPT, 0), before)
        assert fused(product, c) == 1
    finally:
        c.free()
