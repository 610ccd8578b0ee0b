"""gpu: block-int4 models on the bf16 stream kernel of 5..64 rows of a tick / 5..88 of a prompt (lh_ctx_set_q4_stream; csrc/kernels_stream_q4b.h, DESIGN 3l
"Native stream kernel") - every comparison is == on bytes, no tolerance anywhere.

Model A is a synthetic model under QuantizeQ4, evaluated with the switch ON; model B is A's ExpandQ4 int8 twin (tests/test_gpu_q4.py's twins).
k_stream_q4b feeds the operands of k_stream_q8b into the same MFMA and fma sequence, so A's logits and cache rows are B's bytes, and A's route trace is
B's entry by entry: k_stream_q4b for k_stream_q8b, MAXT, NCT, KC, XR and the K-split equal, NIMG (a free choice of the smaller ring, no part of the sums)
ignored.  k_expand_q4 appears only directly in front of a launch that reads int8."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q4_ref as Q                    # noqa: E402
import weight_probe_ref as WP         # noqa: E402
from test_gpu_q4 import SHAPE_KW, families, parse_ggjt, poisoned, same, seeded_cache, twins, write_ggjt   # noqa: E402
from llama_go_amd.mlapi import SHAPES, Batch, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def norm_entry(e):
    """a trace entry as the comparison sees it: k_stream_q4b -> k_stream_q8b, NIMG dropped on both sides"""
    m = re.match(r"^k_stream_q[48]b<([0-9,]+)>(/s\d+)$", e)
    if not m:
        return e
    args = m.group(1).split(",")
    assert len(args) == 5, e                    # MAXT, NCT, KC, NIMG, XR
    return f"k_stream_q8b<{','.join(args[:3] + args[4:])}>{m.group(2)}"


def mapped(ta, tb):
    """A's trace without its expansion passes against B's, under norm_entry.  (The decode stream's kernels are traced in their 4-bit forms only, and
    tests/test_gpu_q4.py holds those to B: left out on both sides.)"""
    keep = lambda t: [norm_entry(e) for e in t if not e.startswith(("k_expand_q4", "k_gemv_"))]   # noqa: E731
    na, nb = keep(ta), keep(tb)
    if na != nb:
        print("trace mismatch:", [(i, x, y) for i, (x, y) in enumerate(zip(na + [None] * len(nb), nb + [None] * len(na))) if x != y][:6])
    return na == nb


def expand_runs(trace):
    """[(number of consecutive k_expand_q4 entries, the entry behind them or None)]"""
    runs, k = [], 0
    for e in trace + [None]:
        if e is not None and e.startswith("k_expand_q4"):
            k += 1
        elif k:
            runs.append((k, e))
            k = 0
    return runs


def cache_rows(c, hp, layers, ctx, past, n):
    d = hp.embdSize
    return [c.CacheRead(which, (il * ctx + past) * d, n * d) for which in (0, 1) for il in range(layers)]


# ---- 1. solo Evals ------------------------------------------------------------------------------------------------------------------------------------------
# small: one row tile per workgroup at most, workgroups without a tile | 7Blayer: MAXT 3 with KC 512 up to 16 rows, w1|w3 pairs at MAXT 6, K = 11008 in
# K-split fours; prompts of 65 and 88 rows in two passes, 89 on Prefill | 13Blayer: MAXT 4 / 8.  5, 9, 17, 33, 49: ragged rows, the column clamps.
ROWS = (5, 8, 9, 16, 17, 32, 33, 48, 49, 64)
SOLO = {"small": (2, 96, ROWS, 11), "7Blayer": (2, 192, ROWS + (65, 88, 89), 37), "13Blayer": (1, 64, (8, 33), 11)}


@pytest.fixture(scope="module", params=list(SOLO))
def solo(product, request):
    shape = request.param
    layers, ctx, rows, past = SOLO[shape]
    hp = make_hparams(**SHAPE_KW[shape], layers=layers, ctx=ctx)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    assert ca.q4_stream is False                       # off by default
    ca.SetQ4Stream(True)
    assert ca.q4_stream is True and cb.q4_stream is False and ca.f16_stream is False
    seeded_cache((ca, cb), hp, layers, ctx)
    yield shape, hp, ca, cb
    ca.free(); cb.free(); A.free(); B.free()


def test_solo_evals_are_byte_equal_and_take_the_twins_kernels(solo):
    shape, hp, ca, cb = solo
    layers, ctx, rows, past1 = SOLO[shape]
    for n in rows:
        rng = np.random.default_rng(100 + n)
        for past in (0, past1):
            toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
            lb, tb = route_trace(lambda: cb.Eval(toks, past))
            assert np.isfinite(lb).all() and np.abs(lb).max() > 0
            assert same(la, lb), (shape, n, past, float(np.abs(la - lb).max()))
            for ra, rb in zip(cache_rows(ca, hp, layers, ctx, past, n), cache_rows(cb, hp, layers, ctx, past, n)):
                assert same(ra, rb), (shape, n, past)
            assert mapped(ta, tb), (shape, n, past, ta, tb)
            fa, fb = families(ta), families(tb)
            assert not set(fb) & {"k_stream_q4b", "k_expand_q4"}, tb
            if n <= 88:      # Planes: every matrix, the output matrix included, is read 4-bit - no expansion pass at all
                assert "k_stream_q8b" in fb and "k_stream_q4b" in fa and "k_stream_q8b" not in fa and "k_expand_q4" not in fa, (shape, n, past, ta)
                assert fa.count("k_stream_q4b") == fb.count("k_stream_q8b") >= 4 * layers * (2 if n > 64 else 1) + 1, (shape, n, past, ta)
            else:            # Prefill keeps the expanded image: each matrix once, directly in front of the launch that reads it (wq|wk|wv, wo, w1|w3, w2)
                assert not set(fa) & {"k_stream_q4b", "k_stream_q8b"}, ta
                runs = expand_runs(ta)
                # (the one logits row llama.Eval reads rides the decode stream on the nibbles: no pass for the output matrix; all rows would add one)
                assert [k for k, _ in runs] in ([3, 1, 2, 1] * layers, [3, 1, 2, 1] * layers + [1]), (shape, n, past, ta)
                # (k_gemm_q8b3 has its own plane split of the activation rows in front: part of that launch)
                assert all(nxt is not None and nxt.startswith(("k_gemm_q8", "k_split3_rows")) for _, nxt in runs), (shape, n, past, ta)


def test_switch_off_is_the_expanded_route(solo):
    shape, hp, ca, cb = solo
    layers = SOLO[shape][0]
    toks = [int(t) for t in np.random.default_rng(7).integers(0, hp.vocabSize, 17)]
    la_on = poisoned(ca).Eval(toks, 0)
    ca.SetQ4Stream(False)
    try:
        assert ca.q4_stream is False
        la, ta = route_trace(lambda: poisoned(ca).Eval(toks, 0))
    finally:
        ca.SetQ4Stream(True)
    lb, tb = route_trace(lambda: cb.Eval(toks, 0))
    fa = families(ta)
    assert same(la, lb) and same(la, la_on)
    assert fa[0] == "k_expand_q4" and fa.count("k_expand_q4") == 7 * layers + 1 and "k_stream_q4b" not in fa, ta
    assert [k for k, _ in expand_runs(ta)] == [7] * layers + [1], ta                  # seven matrices in front of each layer, the output matrix
    assert [e for e in ta if not e.startswith(("k_expand_q4", "k_gemv_"))] == [e for e in tb if not e.startswith("k_gemv_")]   # the parent's launches


# ---- 2. shapes without a k_stream_q8b schedule: the switch changes nothing ------------------------------------------------------------------------------------
# (odd640 itself - ff 1712, no multiple of 32 - cannot be a block-int4 model at all, QuantizeQ4 refuses it; odd640m32 is that shape with ff 1728: a multiple
#  of 32 and not of 128, so q8b_shape_ok is false - the shape tests/test_gpu_q4.py uses for the same reason.  65Blayer: w1|w3 has no k_stream_q8b launch.)
@pytest.mark.parametrize("shape,layers", [("odd640m32", 2), ("65Blayer", 1)])
def test_shapes_the_stream_schedule_is_not_built_for(product, shape, layers):
    ctx = 64
    hp = make_hparams(**SHAPE_KW[shape], layers=layers, ctx=ctx)
    A, B = twins(product, hp)
    con, coff, cb = A.NewContext(ctx, 1), A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    con.SetQ4Stream(True)
    seeded_cache((con, coff, cb), hp, layers, ctx)
    rng = np.random.default_rng(21)
    try:
        for n in (5, 9, 17):
            for past in (0, 11):
                toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
                l1, t1 = route_trace(lambda: con.Eval(toks, past))
                l0, t0 = route_trace(lambda: coff.Eval(toks, past))
                lb = cb.Eval(toks, past)
                assert same(l1, l0) and same(l1, lb), (shape, n, past)
                assert t1 == t0 and not set(families(t1)) & {"k_stream_q4b", "k_stream_q8b"}, (shape, n, past, t1, t0)
                for r1, r0, rb in zip(cache_rows(con, hp, layers, ctx, past, n), cache_rows(coff, hp, layers, ctx, past, n), cache_rows(cb, hp, layers, ctx, past, n)):
                    assert same(r1, r0) and same(r1, rb), (shape, n, past)
    finally:
        con.free(); coff.free(); cb.free(); A.free(); B.free()


# ---- 3. blocks the quantiser never emits ---------------------------------------------------------------------------------------------------------------------
def test_raw_blocks_nibble_zero_all_fifteen_zero_and_nan_scales(product, tmp_path):
    """QuantizeQ4 emits no nibble 0 (q = -8) and no NaN scale.  A saved Q4_0 file is rewritten with such blocks - whole rows of nibble 0 and of nibble 15,
    zero scales, one NaN scale in one block of the output matrix - and loaded back: the registration path of raw 20-byte blocks."""
    ctx = 64
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=ctx)
    src = product.NewSyntheticModel(hp, 77).QuantizeQ4()
    good = str(tmp_path / "small_q4.bin")
    src.SaveQ4(good)
    src.free()
    _, tensors, head = parse_ggjt(good)
    rng = np.random.default_rng(8)
    nan_row = 5
    for name in ("layers.0.attention.wq.weight", "layers.0.attention.wo.weight", "layers.1.feed_forward.w1.weight", "layers.1.feed_forward.w2.weight", "output.weight"):
        dtype, ne, raw = tensors[name]
        assert dtype == 2
        d, n = Q.from_blocks(np.frombuffer(raw, np.uint8), ne[1], ne[0])
        d, n = d.copy(), n.copy()
        n[0::7] = 0                                         # rows of nibble 0: q = -8, which the quantiser never emits
        n[1::7] = 15                                        # rows of all-15
        n[2::7] = rng.integers(0, 16, n[2::7].shape)        # every nibble value next to its neighbours
        d[3::7, ::2] = 0.0                                  # zero scales
        d[4::7, 1] = -0.0
        if name == "output.weight":
            d[nan_row, 3] = np.float32(np.nan)              # one NaN scale in one block: one NaN logit
        tensors[name] = (dtype, ne, Q.to_blocks(d, n).tobytes())
    odd = str(tmp_path / "odd_q4.bin")
    write_ggjt(odd, head, tensors)
    A, B = product.LoadModelKeepQ4(odd, ctx), product.LoadModelKeepQ4(odd, ctx)
    B.ExpandQ4()
    assert A.weight_type == 2 and B.weight_type == 7
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetQ4Stream(True)
    seeded_cache((ca, cb), hp, 2, ctx)
    try:
        for n, past in ((5, 0), (16, 3), (33, 7)):
            toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
            lb, tb = route_trace(lambda: cb.Eval(toks, past))
            la, lb = np.asarray(la).reshape(-1, hp.vocabSize), np.asarray(lb).reshape(-1, hp.vocabSize)
            assert np.isnan(lb[:, nan_row]).all() and np.isfinite(np.delete(lb, nan_row, axis=1)).all() and np.abs(np.nan_to_num(lb)).max() > 0
            assert same(la, lb), (n, past)                   # NaNs by bit pattern
            for ra, rb in zip(cache_rows(ca, hp, 2, ctx, past, n), cache_rows(cb, hp, 2, ctx, past, n)):
                assert same(ra, rb), (n, past)
            assert "k_stream_q4b" in families(ta) and "k_expand_q4" not in families(ta) and mapped(ta, tb), (ta, tb)
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 4. the environment ------------------------------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path.insert(0, {root!r})
from llama_go_amd.mlapi import SHAPES, load_product, make_hparams
p = load_product()
m = p.NewSyntheticModel(make_hparams(**SHAPES["tiny"], ctx=16), 3)
c = m.NewContext(16, 1)
first = c.q4_stream
c.SetQ4Stream(not first)
print("q4_stream", int(first), int(c.q4_stream), int(c.f16_stream))
c.free(); m.free()
"""


@pytest.mark.parametrize("value,want", [("1", 1), ("0", 0), (None, 0)])
def test_environment_sets_the_initial_value_in_a_fresh_process(value, want):
    env = {k: v for k, v in os.environ.items() if k not in ("LLAMAHIP_Q4_STREAM", "LLAMAHIP_ROUTE_FILE")}
    if value is not None:
        env["LLAMAHIP_Q4_STREAM"] = value
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-4:] == ["q4_stream", str(want), str(1 - want), "0"], r.stdout     # read at lh_ctx_create; the setter overrides it


# ---- 5. batches --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_twins(product):
    hp = make_hparams(**SHAPES["small"], ctx=64)
    A, B = twins(product, hp, seed=1234)
    yield hp, A, B
    A.free(); B.free()


def three_legs(small_twins, pods, fn):
    """fn(batch) on A with the switch on, on A with it off, and on the int8 twin"""
    hp, A, B = small_twins
    res = []
    for m, on in ((A, True), (A, False), (B, False)):
        b = Batch(m, 64, pods)
        try:
            assert b.batched, "these shapes must take the one-pass route"
            assert b.q4_stream is False
            if on:
                b.SetQ4Stream(True)
            assert b.q4_stream is on
            res.append(route_trace(lambda: fn(b)))
        finally:
            b.free()
    return res


@pytest.mark.parametrize("pods", [5, 16])
def test_greedy_ticks(small_twins, pods):
    hp = small_twins[0]
    rng = np.random.default_rng(60 + pods)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 2 + i % 3)] for i in range(pods)]
    ((i1, l1), t1), ((i0, l0), t0), ((ib, lb), tb) = three_legs(small_twins, pods, lambda b: poisoned(b, b.model.weight_type == 2).GreedyDecode(prompts, 5, want_logits=True))   # four ticks: eager, captured, replayed twice
    assert i1 == i0 == ib and same(l1, lb) and same(l0, lb)
    assert "k_stream_q4b" in families(t1) and "k_expand_q4" not in families(t1) and mapped(t1, tb), (t1, tb)
    assert "k_stream_q4b" not in families(t0) and "k_expand_q4" in families(t0) and mapped(t0, tb), (t0, tb)


@pytest.mark.parametrize("pods", [5, 16])
def test_sampled_ticks(small_twins, pods):
    hp = small_twins[0]
    rng = np.random.default_rng(65 + pods)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 3)] for _ in range(pods)]

    def run(b):
        first = poisoned(b, b.model.weight_type == 2).Prompt(prompts)
        b.SetSampler(topK=40, seed=9)
        return poisoned(b, b.model.weight_type == 2).Decode(first, [3] * pods, 4, want_logits=True)
    ((i1, l1), t1), ((i0, l0), _), ((ib, lb), tb) = three_legs(small_twins, pods, run)
    assert i1 == i0 == ib and same(l1, lb) and same(l0, lb)
    assert "k_stream_q4b" in families(t1) and mapped(t1, tb), (t1, tb)


def test_feed_of_a_joining_prompt(small_twins):
    hp = small_twins[0]
    pods = 5
    rng = np.random.default_rng(70)
    toks = [[int(t) for t in rng.integers(0, hp.vocabSize, 3)] for _ in range(pods)]
    join = [[int(t) for t in rng.integers(0, hp.vocabSize, 24)]] + [[]] * (pods - 1)          # one pod joins with a 24-token prompt

    def run(b):
        first = poisoned(b, b.model.weight_type == 2).Feed(toks, [0] * pods, want_logits=True, want_rows=True)                     # 15 rows in one pass
        second = poisoned(b, b.model.weight_type == 2).Feed(join, [3] + [0] * (pods - 1), want_logits=True, want_rows=True)        # 24 rows of one pod at past 3
        return first, second
    ((f1, s1), t1), ((f0, s0), _), ((fb, sb), tb) = three_legs(small_twins, pods, run)
    for x, y in ((f1, fb), (s1, sb), (f0, fb), (s0, sb)):
        assert x[0] == y[0] and same(x[1][~np.isnan(y[1]).any(axis=1)], y[1][~np.isnan(y[1]).any(axis=1)]) and same(x[2], y[2])
    assert families(t1).count("k_stream_q4b") >= 2 * (4 * hp.layersCount + 1) and "k_expand_q4" not in families(t1) and mapped(t1, tb), (t1, tb)


def test_lookup_passes_of_sixteen_rows(small_twins):
    hp = small_twins[0]
    pods, R = 4, 4                                       # pods x R = 16 rows per verify pass
    rng = np.random.default_rng(75)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 6)] for _ in range(pods)]

    def run(b):
        first = poisoned(b, b.model.weight_type == 2).Prompt(prompts)
        return poisoned(b, b.model.weight_type == 2).DecodeLookup(first, [6] * pods, 12, R - 1, want_logits=True)
    ((i1, l1, s1, p1), t1), ((i0, l0, s0, p0), _), ((ib, lb, sb, pb), tb) = three_legs(small_twins, pods, run)
    assert i1 == i0 == ib and same(l1, lb) and same(l0, lb) and s1 == s0 == sb and p1 == p0 == pb
    assert any(e.startswith("k_stream_q4b<") and e[e.index("<") + 1:e.index(">")].split(",")[4] == "16" for e in t1), t1   # a 16-row pass (XR = 16) on the 4-bit kernel
    assert mapped(t1, tb), (t1, tb)


def test_toggle_between_ticks_captures_anew(small_twins):
    hp, A, B = small_twins
    pods = 5
    rng = np.random.default_rng(80)
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 3)] for _ in range(pods)]
    ba, bb = Batch(A, 64, pods), Batch(B, 64, pods)
    try:
        first = poisoned(ba).Prompt(prompts)
        assert first == bb.Prompt(prompts)
        past = [3] * pods
        for seg, on in enumerate((False, True, False, False)):
            ba.SetQ4Stream(on)
            assert ba.q4_stream is on
            (ia, la), ta = route_trace(lambda: poisoned(ba).Decode(first, past, 3, want_logits=True))
            ib, lb = bb.Decode(first, past, 3, want_logits=True)
            assert ia == ib and same(la, lb), seg
            fa = families(ta)
            if seg < 3:      # a changed switch (or the first tick): the tick runs eagerly once and is captured anew - its launches are traced twice
                assert ("k_stream_q4b" in fa) == on and ("k_stream_q8b" in fa) == (not on), (seg, ta)
                assert (fa.count("k_expand_q4") == 0) if on else (fa.count("k_expand_q4") >= 2 * 7 * hp.layersCount), (seg, ta)
                streams = [f for f in fa if f.startswith("k_stream_")]
                assert len(streams) >= 2 and len(streams) % 2 == 0 and streams[:len(streams) // 2] == streams[len(streams) // 2:], (seg, ta)
            else:            # the same value again: no change, the captured tick is replayed
                assert not [f for f in fa if f.startswith("k_stream_")], (seg, ta)
            first, past = [r[-1] for r in ia], [p + 3 for p in past]
    finally:
        ba.free(); bb.free()


def test_score_over_forty_tokens(small_twins):
    hp, A, B = small_twins
    toks = [int(t) for t in np.random.default_rng(3).integers(0, hp.vocabSize, 40)]
    res = []
    for m, on in ((A, True), (A, False), (B, False)):
        c = m.NewContext(64, 1)
        try:
            c.SetQ4Stream(on)
            res.append(route_trace(lambda: c.Score(toks, 0)))
        finally:
            c.free()
    (s1, t1), (s0, _), (sb, tb) = res
    assert same(s1, sb) and same(s0, sb)
    assert "k_stream_q4b" in families(t1) and "k_expand_q4" not in families(t1) and mapped(t1, tb), (t1, tb)


# ---- 6. indifference: the switch on plans of another weight type --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "q8"])
def test_switch_does_nothing_for_fp32_and_block_int8(product, kind):
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=64)
    m = product.NewSyntheticModel(hp, 9)
    if kind == "q8":
        m.QuantizeQ8()
    rng = np.random.default_rng(90)
    cases = [([int(t) for t in rng.integers(0, hp.vocabSize, n)], past) for n, past in ((9, 0), (17, 0), (5, 17), (1, 22))]
    res = []
    try:
        for on in (False, True):
            c = m.NewContext(64, 1)
            try:
                c.SetQ4Stream(on)
                assert c.q4_stream is on
                res.append([route_trace(lambda: c.Eval(toks, past)) for toks, past in cases])
            finally:
                c.free()
        for (l0, t0), (l1, t1) in zip(*res):
            assert same(l0, l1) and t0 == t1 and not set(families(t1)) & {"k_stream_q4b", "k_expand_q4"}, (t0, t1)
    finally:
        m.free()
