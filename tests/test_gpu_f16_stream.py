"""gpu: f16 models on the weight-stream MFMA kernels of 2..128 rows (lh_ctx_set_f16_stream; csrc/kernels_stream_f16.h, DESIGN 3k "Native stream kernels") -
every comparison is == on bytes, no tolerance anywhere.

Model A is a synthetic model narrowed with NarrowF16, evaluated with the switch ON; model B is the same seed narrowed and widened again: an fp32 model
(tests/test_gpu_f16.py's twins).  k_stream_mm2_h / k_stream_dma_h feed the fp32 operands of k_stream_mm2 / k_stream_dma into the same MFMA sequence, so A's
logits and cache rows are B's bytes, and A's route trace is B's entry by entry: the _h name for the plain one, MAXT, NCT, KC, CS and the K-split equal,
NIMG and PIPE (free choices of the halved ring, not part of the sums) ignored.  k_widen_f16 appears only directly in front of a launch that reads fp32."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as WP         # noqa: E402
from test_gpu_f16 import families, poisoned, same, seeded_cache, twins   # noqa: E402
from llama_go_amd.mlapi import SHAPES, Batch, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
H_KERNELS = ("k_stream_mm2_h", "k_stream_dma_h")
SHAPE_KW = dict(WP.SHAPES, odd640v516=dict(WP.SHAPES["odd640"], vocab=516))


def norm_entry(e):
    """a trace entry as the comparison sees it: _h -> plain, k_stream_dma's NIMG and PIPE dropped"""
    m = re.match(r"^(k_stream_(?:mm2|dma))(_h)?<([0-9,]+)>(/s\d+)$", e)
    if not m:
        return e
    args = m.group(3).split(",")
    if m.group(1) == "k_stream_dma":
        assert len(args) == 6, e
        args = args[:3] + args[5:]          # MAXT, NCT, KC, CS
    return f"{m.group(1)}<{','.join(args)}>{m.group(4)}"


def mapped(ta, tb):
    """A's trace without its widening passes against B's, under norm_entry.  (The decode stream's kernels - one logits row, the prompts of a batch - are
    traced in their f16 forms only, and tests/test_gpu_f16.py holds those to B: left out on both sides.)"""
    keep = lambda t: [norm_entry(e) for e in t if not e.startswith(("k_widen_f16", "k_gemv_"))]   # noqa: E731
    na, nb = keep(ta), keep(tb)
    if na != nb:
        print("trace mismatch:", [(i, x, y) for i, (x, y) in enumerate(zip(na + [None] * len(nb), nb + [None] * len(na))) if x != y][:6])
    return na == nb


def widen_runs(trace):
    """[(number of consecutive k_widen_f16 entries, the entry behind them or None)]"""
    runs, k = [], 0
    for e in trace + [None]:
        if e is not None and e.startswith("k_widen_f16"):
            k += 1
        elif k:
            runs.append((k, e))
            k = 0
    return runs


def cache_rows(c, hp, layers, ctx, past, n):
    d = hp.embdSize
    return [c.CacheRead(which, (il * ctx + past) * d, n * d) for which in (0, 1) for il in range(layers)]


# ---- 1. solo Evals on the 7B layer shape --------------------------------------------------------------------------------------------------------------
BIG_CTX = 192
# 9, 16: k_stream_mm2(_h), folded norm | 17..48: k_stream_dma(_h), K-split pairs for wo / w2 | 64: Planes (k_stream_b9 over the widened image, unchanged) |
# 65..128: five to eight column tiles (CS = 2 at eight) | 129, 192: two passes
BIG_ROWS = (9, 16, 17, 32, 33, 48, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 192)


@pytest.fixture(scope="module")
def big(product):
    hp = make_hparams(**WP.SHAPES["7Blayer"], layers=2, ctx=BIG_CTX)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(BIG_CTX, 1), B.NewContext(BIG_CTX, 1)
    assert ca.f16_stream is False                      # off by default
    ca.SetF16Stream(True)
    assert ca.f16_stream is True and cb.f16_stream is False
    seeded_cache((ca, cb), hp, 2, BIG_CTX)
    yield hp, ca, cb
    ca.free(); cb.free(); A.free(); B.free()


@pytest.mark.parametrize("n", BIG_ROWS)
def test_solo_evals_are_byte_equal_and_take_the_twins_kernels(big, n):
    hp, ca, cb = big
    rng = np.random.default_rng(100 + n)
    for past in (0, 37):
        if past + n > BIG_CTX:
            continue
        toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
        la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
        lb, tb = route_trace(lambda: cb.Eval(toks, past))
        assert np.isfinite(lb).all() and np.abs(lb).max() > 0
        assert same(la, lb), (n, past, float(np.abs(la - lb).max()))
        for ra, rb in zip(cache_rows(ca, hp, 2, BIG_CTX, past, n), cache_rows(cb, hp, 2, BIG_CTX, past, n)):
            assert same(ra, rb), (n, past)
        assert mapped(ta, tb), (n, past, ta, tb)
        fa = families(ta)
        assert not set(families(tb)) & set(H_KERNELS + ("k_widen_f16",)), tb
        if n == 64:      # Planes keeps the widened image: seven matrices per layer in front of the layer's launches
            assert fa[0] == "k_widen_f16" and fa.count("k_widen_f16") >= 14 and not set(fa) & set(H_KERNELS), ta
        else:
            assert set(fa) & set(H_KERNELS) and not set(fa) & {"k_stream_mm2", "k_stream_dma"}, ta
            # no widening in front of a layer: at most one pass, the output matrix in front of the lm_head, behind every stream launch
            assert fa.count("k_widen_f16") <= 1, ta
            if "k_widen_f16" in fa:
                assert fa.index("k_widen_f16") > max(i for i, f in enumerate(fa) if f in H_KERNELS), ta


def test_switch_off_is_the_widened_route(big):
    hp, ca, cb = big
    toks = [int(t) for t in np.random.default_rng(7).integers(0, hp.vocabSize, 17)]
    ca.SetF16Stream(False)
    try:
        la, ta = route_trace(lambda: poisoned(ca).Eval(toks, 0))
    finally:
        ca.SetF16Stream(True)
    lb, tb = route_trace(lambda: cb.Eval(toks, 0))
    fa = families(ta)
    assert same(la, lb)
    assert fa[0] == "k_widen_f16" and fa.count("k_widen_f16") >= 14 and not set(fa) & set(H_KERNELS), ta
    assert [e for e in ta if not e.startswith(("k_widen_f16", "k_gemv_"))] == [e for e in tb if not e.startswith("k_gemv_")]   # the parent's launches


# ---- 2. small shapes: few tiles per matrix (workgroups without a tile), rows off 16 (column clamps), stream launches next to fallbacks ----------------
@pytest.mark.parametrize("shape,layers", [("small", 2), ("odd640", 2), ("odd640v516", 2), ("65Blayer", 1)])
def test_small_shapes_and_mixed_layers(product, shape, layers):
    ctx = 64
    hp = make_hparams(**SHAPE_KW[shape], layers=layers, ctx=ctx)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetF16Stream(True)
    seeded_cache((ca, cb), hp, layers, ctx)
    rng = np.random.default_rng(21)
    streamed = mixed = 0
    try:
        for n in ((9, 17) if shape == "65Blayer" else (2, 3, 4, 5, 6, 7, 8, 9, 17, 33)):
            for past in (0, 11):
                toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
                lb, tb = route_trace(lambda: cb.Eval(toks, past))
                la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
                assert same(la, lb), (shape, n, past, float(np.abs(la - lb).max()))
                for ra, rb in zip(cache_rows(ca, hp, layers, ctx, past, n), cache_rows(cb, hp, layers, ctx, past, n)):
                    assert same(ra, rb), (shape, n, past)
                fb = families(tb)
                if not set(fb) & {"k_stream_mm2", "k_stream_dma"}:
                    continue                                   # (Rows, Skinny, or no stream launch for the shape: nothing of this file runs)
                streamed += 1
                assert mapped(ta, tb), (shape, n, past, ta, tb)
                assert set(families(ta)) & set(H_KERNELS) and not set(families(ta)) & {"k_stream_mm2", "k_stream_dma"}, ta
                # a widening pass stands only directly in front of a launch that reads fp32, and only for the matrices it reads (<= 3 per launch)
                runs = widen_runs(ta)
                for k, nxt in runs:
                    assert nxt is not None and not nxt.startswith("k_stream_") and k <= 3, (shape, n, past, ta)
                if any(not f.startswith("k_stream") and f != "k_widen_f16" for f in fb[:-1]):
                    mixed += 1
                if shape == "65Blayer":
                    # w1|w3 (twelve tile pairs per workgroup: not built) is the one fallback of the layer: exactly its two matrices, then at most the output matrix
                    assert [k for k, _ in runs[:1]] == [2] and len(runs) <= 2 and (len(runs) == 1 or runs[1][0] == 1), (n, past, ta)
        assert streamed >= 2, shape
        if shape == "65Blayer":
            assert mixed >= 1
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 3. values: every subnormal half, +-0 and the largest finite halves inside the stream kernels --------------------------------------------------------
def value_matrix(rows, cols):
    n = rows * cols
    pat = (np.arange(n, dtype=np.int64) % 1100 + 1).astype(np.uint16)            # 0x0001 .. 0x044C: all 1023 subnormals and the smallest normals
    pat[5::1100] = 0x0000                                                        # +0 (-0 through the alternating sign below)
    pat[6::1100] = 0x0000
    pat[17::2200] = 0x7BFF                                                       # 65504, the largest finite half, both signs (odd and even positions)
    pat[18::2200] = 0x7BFF
    halves = pat | ((np.arange(n) & 1).astype(np.uint16) << 15)                  # alternating sign
    return halves.view(np.float16).astype(np.float32).reshape(rows, cols)


def test_subnormals_zeros_and_the_largest_halves(product):
    kw = WP.SHAPES["small"]
    ctx = 64
    hp = make_hparams(**kw, layers=2, ctx=ctx)
    d = kw["embd"]
    F = ((2 * (4 * d) // 3 + kw["mult"] - 1) // kw["mult"]) * kw["mult"]      # llama.go:210-211
    wq, w2 = value_matrix(d, d), value_matrix(d, F)
    assert int((np.abs(wq) < 2.0 ** -14).sum()) > d * d // 2 and np.isfinite(wq).all() and float(np.abs(wq).max()) == 65504.0
    flush = lambda w: np.where(np.abs(w) < 2.0 ** -14, np.float32(0), w)   # noqa: E731

    def put(m, a, b):
        m.SetTensor("layers.0.attention.wq.weight", a)
        m.SetTensor("layers.0.feed_forward.w2.weight", b)

    A, B = twins(product, hp, prepare=lambda m: put(m, wq, w2))
    Cm = product.NewSyntheticModel(hp, 77)                                  # B with the subnormals flushed to zero: what a flushing conversion would compute
    Cm.NarrowF16(); Cm.WidenF16()
    put(Cm, flush(wq), flush(w2))
    ca, cb, cc = A.NewContext(ctx, 1), B.NewContext(ctx, 1), Cm.NewContext(ctx, 1)
    ca.SetF16Stream(True)
    rng = np.random.default_rng(31)
    try:
        for n in (9, 17):                                                    # conversion in the loader waves (k_stream_mm2_h) / in the MFMA waves (k_stream_dma_h)
            toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, 0))
            lb, lc = cb.Eval(toks, 0), cc.Eval(toks, 0)
            assert H_KERNELS[0 if n == 9 else 1] in families(ta), ta
            assert np.isfinite(lb).all()
            assert same(la, lb), (n, float(np.abs(la - lb).max()))
            assert not same(la, lc), n                                       # the subnormals reach the logits
    finally:
        ca.free(); cb.free(); cc.free(); A.free(); B.free(); Cm.free()


# ---- 4. batches -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_twins(product):
    hp = make_hparams(**SHAPES["small"], ctx=64)
    A, B = twins(product, hp, seed=1234)
    yield hp, A, B
    A.free(); B.free()


@pytest.mark.parametrize("pods", [9, 16, 17, 32, 33, 48])
def test_batch_ticks(small_twins, pods):
    hp, A, B = small_twins
    rng = np.random.default_rng(60 + pods)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 2 + i % 3)] for i in range(pods)]
    res = []
    for m in (A, B):
        b = Batch(m, 64, pods)
        try:
            assert b.batched, "these shapes must take the one-pass route"
            if m is A:
                b.SetF16Stream(True)
                assert b.f16_stream is True
            (ids, lg), tr = route_trace(lambda: poisoned(b, m is A).GreedyDecode(prompts, 5, want_logits=True))   # four ticks: eager, captured, replayed twice
            res.append((ids, lg, tr))
        finally:
            b.free()
    (ia, la, ta), (ib, lb, tb) = res
    assert ia == ib and same(la, lb)
    assert set(families(ta)) & set(H_KERNELS), ta
    assert mapped(ta, tb), (ta, tb)


def test_batch_feed(small_twins):
    hp, A, B = small_twins
    rng = np.random.default_rng(70)
    toks = [[int(t) for t in rng.integers(0, hp.vocabSize, 5)] for _ in range(3)]
    more = [[int(t) for t in rng.integers(0, hp.vocabSize, 4)] for _ in range(3)]
    res = []
    for m in (A, B):
        b = Batch(m, 64, 3)
        try:
            if m is A:
                b.SetF16Stream(True)
            first, t1 = route_trace(lambda: poisoned(b, m is A).Feed(toks, [0, 0, 0], want_logits=True, want_rows=True))      # 15 rows in one pass
            second, t2 = route_trace(lambda: poisoned(b, m is A).Feed(more, [5, 5, 5], want_logits=True, want_rows=True))     # 12 rows at past > 0
            res.append((first, second, t1 + t2))
        finally:
            b.free()
    (fa, sa, ta), (fb, sb, tb) = res
    for x, y in ((fa, fb), (sa, sb)):
        assert x[0] == y[0] and same(x[1], y[1]) and same(x[2], y[2])
    assert "k_stream_mm2_h" in families(ta) and mapped(ta, tb), (ta, tb)


def test_toggle_between_ticks_captures_anew(small_twins):
    hp, A, B = small_twins
    pods = 9
    rng = np.random.default_rng(80)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 3)] for _ in range(pods)]
    ba, bb = Batch(A, 64, pods), Batch(B, 64, pods)
    try:
        first = poisoned(ba).Prompt(prompts)
        assert first == bb.Prompt(prompts)
        past = [3] * pods
        for seg, on in enumerate((False, True, False, False)):
            ba.SetF16Stream(on)
            assert ba.f16_stream is on
            (ia, la), ta = route_trace(lambda: poisoned(ba).Decode(first, past, 3, want_logits=True))
            ib, lb = bb.Decode(first, past, 3, want_logits=True)
            assert ia == ib and same(la, lb), seg
            fa = families(ta)
            if seg < 3:      # a changed switch: the tick runs eagerly once and is captured anew - its launches are traced twice
                assert bool(set(fa) & set(H_KERNELS)) == on, (seg, ta)
                assert fa.count("k_widen_f16") >= (0 if on else 2 * 7 * hp.layersCount), (seg, ta)
                streams = [f for f in fa if f.startswith("k_stream_")]
                assert len(streams) >= 2 and len(streams) % 2 == 0 and streams[:len(streams) // 2] == streams[len(streams) // 2:], (seg, ta)
            else:            # the same value again: no change, the captured tick is replayed
                assert not [f for f in fa if f.startswith("k_stream_")], (seg, ta)
            first, past = [r[-1] for r in ia], [p + 3 for p in past]
    finally:
        ba.free(); bb.free()


# ---- 5. indifference: the switch on plans of another weight type --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quant", [False, True])
def test_switch_does_nothing_for_fp32_and_block_int8(product, quant):
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=64)
    m = product.NewSyntheticModel(hp, 9)
    if quant:
        m.QuantizeQ8()
    rng = np.random.default_rng(90)
    cases = [([int(t) for t in rng.integers(0, hp.vocabSize, n)], past) for n, past in ((9, 0), (17, 0), (5, 17), (1, 22))]
    res = []
    try:
        for on in (False, True):
            c = m.NewContext(64, 1)
            try:
                if on:
                    c.SetF16Stream(True)
                assert c.f16_stream is on
                res.append([route_trace(lambda: c.Eval(toks, past)) for toks, past in cases])
            finally:
                c.free()
        for (l0, t0), (l1, t1) in zip(*res):
            assert same(l0, l1) and t0 == t1 and not set(families(t1)) & set(H_KERNELS + ("k_widen_f16",)), (t0, t1)
    finally:
        m.free()
