"""gpu: f16 models on the bf16 tile GEMM of prompts beyond 128 rows (lh_ctx_set_f16_tiles; csrc/kernels_gemm_f16.h, DESIGN 3k "Native tile GEMM") - every
comparison is == on bytes, no tolerance anywhere.

Model A is a synthetic model narrowed with NarrowF16, evaluated with the switch ON; model B is the same seed narrowed and widened again: an fp32 model
(tests/test_gpu_f16.py's twins).  k_gemm_b9_h issues k_gemm_b9's products without the two that read the weights' third bf16 part - exact zeros for every
finite half - so A's logits and cache rows are B's bytes, and A's route trace is B's entry by entry: k_gemm_b9_h<1,8,4,1,NST>/sS for
k_gemm_b9<1,8,4,1,2>/sS (the ring depth is no part of the sums), the split count equal.  k_widen_f16 appears only directly in front of a launch that reads
fp32, never in front of a k_gemm_b9_h."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as WP         # noqa: E402
from test_gpu_f16 import families, poisoned, same, seeded_cache, twins   # noqa: E402
from test_gpu_f16_stream import widen_runs   # noqa: E402
from llama_go_amd.mlapi import make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
H = "k_gemm_b9_h"
HALF_READERS = (H, "k_stream_mm2_h", "k_stream_dma_h", "k_gemv_sa_h", "k_gemv_rows_h")


def norm_entry(e):
    """a trace entry as the comparison sees it: k_gemm_b9_h<1,8,4,1,NST>/sS -> k_gemm_b9<1,8,4,1,2>/sS; the stream kernels as tests/test_gpu_f16_stream.py"""
    m = re.match(r"^k_gemm_b9_h<1,8,4,1,\d+>(/s\d+)$", e)
    if m:
        return "k_gemm_b9<1,8,4,1,2>" + m.group(1)
    m = re.match(r"^(k_stream_(?:mm2|dma))(_h)?<([0-9,]+)>(/s\d+)$", e)
    if not m:
        return e
    args = m.group(3).split(",")
    if m.group(1) == "k_stream_dma":
        args = args[:3] + args[5:]
    return f"{m.group(1)}<{','.join(args)}>{m.group(4)}"


def mapped(ta, tb):
    keep = lambda t: [norm_entry(e) for e in t if not e.startswith(("k_widen_f16", "k_gemv_"))]   # noqa: E731
    na, nb = keep(ta), keep(tb)
    if na != nb:
        print("trace mismatch:", [(i, x, y) for i, (x, y) in enumerate(zip(na + [None] * len(nb), nb + [None] * len(na))) if x != y][:6])
    return na == nb


def widening_is_in_front_of_fp32_readers(ta):
    """every run of k_widen_f16 entries stands directly in front of a launch that reads fp32 (k_split3_rows, the activation pass of a k_gemm_b9 launch, may
    stand between), and holds at most the three matrices one launch reads"""
    for i, e in enumerate(ta):
        if not e.startswith("k_widen_f16") or (i + 1 < len(ta) and ta[i + 1].startswith("k_widen_f16")):
            continue
        rest = [x for x in ta[i + 1:] if x != "k_split3_rows"]
        if not rest or rest[0].startswith(HALF_READERS):
            print("a widening pass without an fp32 reader behind it:", i, ta[max(0, i - 3):i + 4])
            return False
    return all(k <= 3 for k, _ in widen_runs(ta))


def count(trace, fam):
    return sum(1 for f in families(trace) if f == fam)


def cache_rows(c, hp, layers, ctx, past, n):
    d = hp.embdSize
    return [c.CacheRead(which, (il * ctx + past) * d, n * d) for which in (0, 1) for il in range(layers)]


def eval_pair(ca, cb, hp, layers, ctx, toks, past):
    la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
    lb, tb = route_trace(lambda: cb.Eval(toks, past))
    n = len(toks)
    assert np.isfinite(lb).all() and np.abs(lb).max() > 0
    assert same(la, lb), (n, past, float(np.abs(la - lb).max()))
    for ra, rb in zip(cache_rows(ca, hp, layers, ctx, past, n), cache_rows(cb, hp, layers, ctx, past, n)):
        assert same(ra, rb), (n, past)
    return ta, tb


def tiles_checks(ta, tb, where):
    assert mapped(ta, tb), (where, ta, tb)
    assert not set(families(tb)) & set(HALF_READERS + ("k_widen_f16",)), tb
    assert count(ta, H) == count(tb, "k_gemm_b9") > 0, (where, ta, tb)
    assert count(ta, "k_gemm_b9") == 0, (where, ta)
    assert widening_is_in_front_of_fp32_readers(ta), (where, ta)


# ---- 1. the 7B layer shape: two / three / four row tiles, the last one of 65 / 1 / 1 rows -------------------------------------------------------------
BIG_CTX = 392


@pytest.fixture(scope="module")
def big(product):
    hp = make_hparams(**WP.SHAPES["7Blayer"], layers=2, ctx=BIG_CTX)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(BIG_CTX, 1), B.NewContext(BIG_CTX, 1)
    assert ca.f16_tiles is False                       # off by default
    ca.SetF16Tiles(True)
    assert ca.f16_tiles is True and cb.f16_tiles is False and ca.f16_stream is False
    seeded_cache((ca, cb), hp, 2, BIG_CTX)
    yield hp, ca, cb
    ca.free(); cb.free(); A.free(); B.free()


@pytest.mark.parametrize("n", [193, 257, 385])
def test_prompts_are_byte_equal_and_take_the_twins_tiles(big, n):
    hp, ca, cb = big
    rng = np.random.default_rng(300 + n)
    for past in (0, 7):
        toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
        ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, toks, past)
        tiles_checks(ta, tb, (n, past))
        if n == 193:      # split-K and its reduce pass are covered: some launches split, some do not
            splits = {int(e.rsplit("/s", 1)[1]) for e in ta if e.startswith(H)}
            assert 1 in splits and max(splits) > 1 and "k_splitk_reduce" in ta, ta
        # every layer matrix went through the half kernel: at most one widening pass, the output matrix, and only if the lm_head is no k_gemm_b9 launch
        assert count(ta, "k_widen_f16") <= 1 and count(ta, H) >= 2 * 4, ta


# ---- 2. ragged M (F % 256 = 192) and an uneven deal of w2's 342 slabs -----------------------------------------------------------------------------------
def test_ragged_m_and_an_uneven_k_deal(product):
    kw = dict(WP.SHAPES["7Blayer"], mult=32)
    ctx = 200
    hp = make_hparams(**kw, layers=1, ctx=ctx)
    F = ((2 * (4 * kw["embd"]) // 3 + kw["mult"] - 1) // kw["mult"]) * kw["mult"]      # llama.go:210-211
    assert F == 10944 and F % 256 == 192 and (F // 32) == 342
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetF16Tiles(True)
    seeded_cache((ca, cb), hp, 1, ctx)
    try:
        toks = [int(t) for t in np.random.default_rng(41).integers(0, hp.vocabSize, 193)]
        ta, tb = eval_pair(ca, cb, hp, 1, ctx, toks, 0)
        gb = [e for e in tb if e.startswith(("k_gemm_", "k_stream_"))]
        gb = gb[:4]                                                                     # wq|wk|wv, wo, w1|w3, w2 (the lm_head behind them)
        assert len(gb) == 4 and all(e.startswith("k_gemm_b9<") for e in gb), tb          # ... all four on k_gemm_b9
        assert int(gb[3].rsplit("/s", 1)[1]) > 1 and 342 % int(gb[3].rsplit("/s", 1)[1]) != 0, gb   # w2's slabs do not divide among its ranges
        tiles_checks(ta, tb, "mult32")
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 3. K = 8192 / 22016 and other split counts ------------------------------------------------------------------------------------------------------
def test_the_65b_layer(product):
    ctx = 200
    hp = make_hparams(**WP.SHAPES["65Blayer"], layers=1, ctx=ctx)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetF16Tiles(True)
    seeded_cache((ca, cb), hp, 1, ctx)
    try:
        toks = [int(t) for t in np.random.default_rng(43).integers(0, hp.vocabSize, 193)]
        ta, tb = eval_pair(ca, cb, hp, 1, ctx, toks, 0)
        tiles_checks(ta, tb, "65Blayer")
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 4. both switches ---------------------------------------------------------------------------------------------------------------------------------
def test_both_switches_and_toggles(big):
    hp, ca, cb = big
    rng = np.random.default_rng(50)
    toks = [int(t) for t in rng.integers(0, hp.vocabSize, 193)]
    try:
        ca.SetF16Stream(True)
        assert ca.f16_stream is True and ca.f16_tiles is True
        ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, toks, 0)
        tiles_checks(ta, tb, "both")
        ca.SetF16Stream(False)
        # tiles on, stream off, 150 rows: the two-pass stream route over lazily widened images - the fp32 stream kernels, each matrix widened once,
        # directly in front of its first reader
        t150 = [int(t) for t in rng.integers(0, hp.vocabSize, 150)]
        ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, t150, 0)
        assert mapped(ta, tb), (ta, tb)
        assert [e for e in ta if not e.startswith(("k_widen_f16", "k_gemv_"))] == [e for e in tb if not e.startswith("k_gemv_")], (ta, tb)   # no _h kernel
        assert set(families(tb)) & {"k_stream_dma", "k_stream_mm2"}, tb
        assert widening_is_in_front_of_fp32_readers(ta), ta
        assert families(ta)[0] == "k_widen_f16" and [k for k, _ in widen_runs(ta)][:8] == [3, 1, 2, 1] * 2 and count(ta, "k_widen_f16") <= 2 * 7 + 1, ta
        # on / off / on between Evals of one context
        for on in (True, False, True):
            ca.SetF16Tiles(on)
            assert ca.f16_tiles is on
            ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, toks, 0)
            assert (count(ta, H) > 0) is on and (count(ta, "k_gemm_b9") == 0) is on, (on, ta)
            assert mapped(ta, tb), (on, ta, tb)
    finally:
        ca.SetF16Stream(False)
        ca.SetF16Tiles(True)


# ---- 5. Score: the lm_head of all 193 rows ---------------------------------------------------------------------------------------------------------------
def test_score_over_193_tokens(big):
    hp, ca, cb = big
    toks = [int(t) for t in np.random.default_rng(60).integers(0, hp.vocabSize, 193)]
    sa, ta = route_trace(lambda: poisoned(ca).Score(toks, 0))
    sb, tb = route_trace(lambda: cb.Score(toks, 0))
    assert len(sa) == 193 and sa.dtype == sb.dtype
    for field in sa.dtype.names:                           # per-row log-probs, argmax, rank ...: every field by bytes
        assert same(sa[field], sb[field]), field
    assert same(sa, sb)
    assert mapped(ta, tb), (ta, tb)
    assert widening_is_in_front_of_fp32_readers(ta), ta
    mm = lambda t: [e for e in t if e.startswith(("k_gemm_", "k_stream_", "k_gemv_"))]   # noqa: E731
    head_a, head_b = mm(ta)[-1], mm(tb)[-1]
    if head_b.startswith("k_gemm_b9<"):                    # the twin's lm_head on k_gemm_b9: A's on the halves, no widening anywhere
        assert head_a.startswith(H + "<") and count(ta, "k_widen_f16") == 0, ta
    else:                                                  # any other launch: exactly one pass, the output matrix, directly in front of it
        assert count(ta, "k_widen_f16") == 1 and ta[ta.index("k_widen_f16") + 1] == head_a and not head_a.startswith(HALF_READERS), ta


# ---- 6. values: every subnormal half, +-0 and the largest finite halves inside the tile kernel -----------------------------------------------------------
def all_values_matrix(rows, cols):
    """tests/test_gpu_f16_stream.py's value_matrix with an odd period, so that every pattern meets both signs and both column parities: all 1023 subnormal
    halves and the smallest normals, +-0, +-65504"""
    n = rows * cols
    idx = np.arange(n, dtype=np.int64)
    pat = (idx % 1101 + 1).astype(np.uint16)            # 0x0001 .. 0x044D
    pat[idx % 1101 >= 1099] = 0x0000                    # two zeros per period
    pat[(idx % 1101 == 1097) | (idx % 1101 == 1098)] = 0x7BFF
    halves = pat | (((idx // 2202) & 1).astype(np.uint16) << 15)  # the sign changes every second period: each pattern with both signs at both parities
    return halves.view(np.float16).astype(np.float32).reshape(rows, cols)


def test_subnormals_zeros_and_the_largest_halves(product):
    kw = WP.SHAPES["7Blayer"]
    ctx = 200
    hp = make_hparams(**kw, layers=1, ctx=ctx)
    d = kw["embd"]
    F = ((2 * (4 * d) // 3 + kw["mult"] - 1) // kw["mult"]) * kw["mult"]      # llama.go:210-211
    wq, w2 = all_values_matrix(d, d), all_values_matrix(d, F)
    for w in (wq, w2):
        assert int((np.abs(w) < 2.0 ** -14).sum()) > w.size // 2 and np.isfinite(w).all() and float(np.abs(w).max()) == 65504.0
        sub = w[(np.abs(w) < 2.0 ** -14) & (w != 0)]
        assert len(np.unique(sub)) == 2 * 1023                                              # every subnormal half, both signs
        for col in (0, 1):                                                                  # +-0 and +-65504 at even and at odd columns
            assert {0x0000, 0x8000, 0x7BFF, 0xFBFF} <= set(np.unique(w[:, col::2].astype(np.float16).view(np.uint16)).tolist())

    def put(m):
        m.SetTensor("layers.0.attention.wq.weight", wq)
        m.SetTensor("layers.0.feed_forward.w2.weight", w2)

    A, B = twins(product, hp, prepare=put)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetF16Tiles(True)
    seeded_cache((ca, cb), hp, 1, ctx)
    try:
        toks = [int(t) for t in np.random.default_rng(31).integers(0, hp.vocabSize, 193)]
        ta, tb = eval_pair(ca, cb, hp, 1, ctx, toks, 0)
        tiles_checks(ta, tb, "values")
        assert count(ta, H) >= 4, ta                        # wq (in wq|wk|wv) and w2 among them
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 7. the switch ------------------------------------------------------------------------------------------------------------------------------------------
def test_off_is_the_parents_route(big):
    hp, ca, cb = big
    toks = [int(t) for t in np.random.default_rng(7).integers(0, hp.vocabSize, 193)]
    ca.SetF16Tiles(False)
    try:
        ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, toks, 0)
    finally:
        ca.SetF16Tiles(True)
    fa = families(ta)
    assert fa[0] == "k_widen_f16" and fa.count("k_widen_f16") >= 14 and H not in fa, ta
    assert [e for e in ta if not e.startswith(("k_widen_f16", "k_gemv_"))] == [e for e in tb if not e.startswith("k_gemv_")]   # the parent's launches


@pytest.mark.parametrize("quant", [False, True])
def test_switch_does_nothing_for_fp32_and_block_int8(product, quant):
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=256)
    m = product.NewSyntheticModel(hp, 9)
    if quant:
        m.QuantizeQ8()
    rng = np.random.default_rng(90)
    cases = [([int(t) for t in rng.integers(0, hp.vocabSize, n)], past) for n, past in ((193, 0), (17, 0), (1, 22))]
    res = []
    try:
        for on in (False, True):
            c = m.NewContext(256, 1)
            try:
                if on:
                    c.SetF16Tiles(True)
                assert c.f16_tiles is on
                res.append([route_trace(lambda: c.Eval(toks, past)) for toks, past in cases])
            finally:
                c.free()
        for (l0, t0), (l1, t1) in zip(*res):
            assert same(l0, l1) and t0 == t1 and not set(families(t1)) & set(HALF_READERS + ("k_widen_f16",)), (t0, t1)
    finally:
        m.free()


def test_environment_sets_the_initial_value(big, product):
    hp, ca, cb = big
    old = os.environ.get("LLAMAHIP_F16_TILES")
    m = product.NewSyntheticModel(make_hparams(**WP.SHAPES["small"], layers=1, ctx=32), 3)
    try:
        for value, want in (("1", True), ("0", False), (None, False)):
            if value is None:
                os.environ.pop("LLAMAHIP_F16_TILES", None)
            else:
                os.environ["LLAMAHIP_F16_TILES"] = value
            c = m.NewContext(32, 1)                          # read once, when the context is created
            try:
                assert c.f16_tiles is want, value
                os.environ["LLAMAHIP_F16_TILES"] = "0" if want else "1"
                assert c.f16_tiles is want                   # ... and not again
                c.SetF16Tiles(not want)
                assert c.f16_tiles is (not want)             # the setter overrides it
            finally:
                c.free()
        assert ca.f16_tiles is True                          # contexts that exist keep their value
    finally:
        if old is None:
            os.environ.pop("LLAMAHIP_F16_TILES", None)
        else:
            os.environ["LLAMAHIP_F16_TILES"] = old
        m.free()
