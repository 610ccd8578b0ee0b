"""gpu: block-int4 models on the bf16 tile GEMM of prompts from 89 rows (lh_ctx_set_q4_tiles; csrc/kernels_gemm_q4.h, DESIGN 3l "Native tile GEMM") - every
comparison with the twin is == on bytes, no tolerance anywhere.

Model A is a synthetic model under QuantizeQ4, evaluated with the switch ON and its weight images poisoned in front of every call; model B is A's ExpandQ4
int8 twin (tests/test_gpu_q4.py's twins).  k_gemm_q4b3 feeds k_gemm_q8b3's operands into the same MFMA and fma sequence, so A's logits and cache rows
are B's bytes and A's route trace is B's entry by entry, k_gemm_q4b3<*> for k_gemm_q8b3<4> with equal split counts; k_expand_q4 appears only directly in
front of a launch that reads int8 (k_gemm_q8)."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q4_ref as Q                    # noqa: E402
import weight_probe_ref as WP         # noqa: E402
from test_gpu_q4 import SHAPE_KW, families, parse_ggjt, poisoned, same, seeded_cache, twins, write_ggjt   # noqa: E402
from test_gpu_q4_stream import cache_rows, expand_runs   # noqa: E402
from test_gpu_weight_probe import run_call               # noqa: E402
from llama_go_amd.mlapi import SHAPES, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mapped(ta, tb):
    """A's trace without its expansion passes against B's with k_gemm_q4b3<*> read as k_gemm_q8b3<4> (the ring depth is no part of the sums); the decode
    stream's kernels are traced in their 4-bit forms only (tests/test_gpu_q4.py holds those to B): left out on both sides"""
    keep = lambda t: [re.sub(r"^k_gemm_q4b3<\d+>", "k_gemm_q8b3<4>", e) for e in t if not e.startswith(("k_expand_q4", "k_gemv_"))]   # noqa: E731
    return keep(ta) == keep(tb)


def tiles_only(ta, tb):
    """A took k_gemm_q4b3 wherever B took k_gemm_q8b3, and expanded only directly in front of a k_gemm_q8 launch"""
    fa, fb = families(ta), families(tb)
    return ("k_gemm_q8b3" in fb and "k_gemm_q4b3" in fa and "k_gemm_q8b3" not in fa and not set(fb) & {"k_gemm_q4b3", "k_expand_q4"}
            and all(nxt is not None and nxt.startswith("k_gemm_q8<") for _, nxt in expand_runs(ta)))


# ---- 1. byte equality and the twin's launches ---------------------------------------------------------------------------------------------------------------
# small: 89 = one ragged row tile, 129 = a second tile of one row | odd640m32: M = 640 / 1728 / 515 ragged against 256, w2 has K = 1728 (no multiple of
# 128): that launch stays k_gemm_q8 behind an expansion | 7Blayer: K = 11008, 86 scale groups dealt unevenly to the split-K ranges
EVALS = {"small": (2, (89, 128, 129, 257)), "odd640m32": (2, (89,)), "7Blayer": (1, (89,))}
SPLITS = set()


@pytest.mark.parametrize("shape", list(EVALS))
def test_evals_are_byte_equal_and_take_the_twins_launches(product, shape):
    layers, rows = EVALS[shape]
    ctx = max(rows) + 7
    hp = make_hparams(**SHAPE_KW[shape], layers=layers, ctx=ctx)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    assert ca.q4_tiles is False                        # off by default
    ca.SetQ4Tiles(True)
    assert ca.q4_tiles is True and cb.q4_tiles is False and ca.q4_stream is False
    seeded_cache((ca, cb), hp, layers, ctx)
    splits = set()
    try:
        for n in rows:
            rng = np.random.default_rng(300 + n)
            for past in (0, 7):
                toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
                la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
                lb, tb = route_trace(lambda: cb.Eval(toks, past))
                assert np.isfinite(lb).all() and np.abs(lb).max() > 0
                assert same(la, lb), (shape, n, past, float(np.abs(la - lb).max()))
                for ra, rb in zip(cache_rows(ca, hp, layers, ctx, past, n), cache_rows(cb, hp, layers, ctx, past, n)):
                    assert same(ra, rb), (shape, n, past)
                assert mapped(ta, tb) and tiles_only(ta, tb), (shape, n, past, ta, tb)
                assert ("k_gemm_q8<" in " ".join(tb)) == (shape == "odd640m32") == bool(expand_runs(ta)), (shape, ta, tb)
                for i, e in enumerate(tb):
                    if e.startswith("k_gemm_q8b3"):
                        s = int(e.rsplit("/s", 1)[1])
                        splits.add(s)
                        assert (s > 1) == (tb[i + 1:i + 2] == ["k_splitk_reduce"]), (e, tb)      # (A's: mapped)
        print(shape, "split counts of k_gemm_q8b3:", sorted(splits))
        SPLITS.update(splits)
        if shape == list(EVALS)[-1]:                   # over the shapes: a launch without split-K and one with (and its k_splitk_reduce)
            assert 1 in SPLITS and max(SPLITS) > 1, SPLITS
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_weight_probe.py's probe layers and calls on a block-int4 model with the switch on (its contexts are made inside run_call: the environment
# switch).  Reference weights: fl32(d (n - 8)) by tests/q4_ref.py's quantiser rule; the bound is weight_probe_ref's own for block-int8 launches - the same
# arithmetic.  (llamago_Stage's head computes ONE logits row - the decode stream; the multi-row head is held by bytes in 3. and 4.)
_REFS = {}


def q4_probe(product, probe):
    if probe not in _REFS:
        kw = WP.SHAPES["small"]
        hp = make_hparams(**kw, layers=3, ctx=WP.CTX)
        layer = 2 if probe == "head" else 1
        m = product.NewSyntheticModel(hp, 7, layer, layer + 1)
        T = WP.probe_tensors(probe, "small")
        names = {k: f"layers.{layer}.{v}" for k, v in WP.TENSOR_NAMES.items()}
        if probe == "head":
            names.update(norm="norm.weight", output="output.weight")
        for k, name in names.items():
            m.SetTensor(name, T[k])
        m.QuantizeQ4()
        W = {}
        for k, w in T.items():
            if k in names and w.ndim == 2:
                d, n = Q.quantize(w)
                w = (d[..., None] * (n.astype(np.float32) - np.float32(8))).astype(np.float32).reshape(w.shape)
            W[k] = w
        X = WP.inputs("small", 129)
        _REFS[probe] = types.SimpleNamespace(probe=probe, model=m, X=X, d=kw["embd"], V=kw["vocab"], ref=WP.reference(probe, W, X))
    return _REFS[probe]


@pytest.fixture(scope="module")
def probe_models():
    yield
    for p in _REFS.values():
        p.model.free()
    _REFS.clear()


@pytest.mark.parametrize("n", [89, 129])
@pytest.mark.parametrize("probe", WP.PROBES)
def test_each_launch_against_float64(product, probe_models, monkeypatch, probe, n):
    monkeypatch.setenv("LLAMAHIP_Q4_TILES", "1")
    P = q4_probe(product, probe)
    y, trace = run_call(product, P, n, 0)
    rows = slice(n - 1, n) if probe == "head" else slice(0, n)
    ref = dict(out=P.ref["out"][rows], bound=P.ref["bound"][rows])
    print(f"{probe} n={n}: error / bound {WP.ratio(y, ref):.4g}; {' '.join(dict.fromkeys(families(trace)))}")
    if probe != "head":
        assert families(trace).count("k_gemm_q4b3") == 4 and not set(families(trace)) & {"k_gemm_q8b3", "k_gemm_q8", "k_expand_q4"}, trace
    err = np.abs(y.astype(np.float64) - ref["out"])
    assert (err <= ref["bound"]).all(), (probe, n, WP.ratio(y, ref))


# ---- 3. blocks the quantiser never emits ------------------------------------------------------------------------------------------------------------------------
def test_raw_blocks_nibble_zero_all_fifteen_zero_and_nan_scales(product, tmp_path):
    """tests/test_gpu_q4_stream.py's construction: a saved Q4_0 file rewritten with rows of nibble 0 (q = -8) and of nibble 15, zero and -0 scales, one NaN
    scale in one block of the output matrix; 89 rows, the all-rows lm_head through Score"""
    ctx = 96
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=ctx)
    src = product.NewSyntheticModel(hp, 77).QuantizeQ4()
    good = str(tmp_path / "small_q4.bin")
    src.SaveQ4(good)
    src.free()
    _, tensors, head = parse_ggjt(good)
    rng = np.random.default_rng(8)
    for name in ("layers.0.attention.wq.weight", "layers.0.attention.wo.weight", "layers.1.feed_forward.w1.weight", "layers.1.feed_forward.w2.weight", "output.weight"):
        dtype, ne, raw = tensors[name]
        assert dtype == 2
        d, n = Q.from_blocks(np.frombuffer(raw, np.uint8), ne[1], ne[0])
        d, n = d.copy(), n.copy()
        n[0::7] = 0
        n[1::7] = 15
        n[2::7] = rng.integers(0, 16, n[2::7].shape)
        d[3::7, ::2] = 0.0
        d[4::7, 1] = -0.0
        if name == "output.weight":
            d[5, 3] = np.float32(np.nan)
        tensors[name] = (dtype, ne, Q.to_blocks(d, n).tobytes())
    odd = str(tmp_path / "odd_q4.bin")
    write_ggjt(odd, head, tensors)
    A, B = product.LoadModelKeepQ4(odd, ctx), product.LoadModelKeepQ4(odd, ctx)
    B.ExpandQ4()
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetQ4Tiles(True)
    seeded_cache((ca, cb), hp, 2, ctx)
    try:
        toks = [int(t) for t in rng.integers(0, hp.vocabSize, 89)]
        for past in (0, 3):
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
            lb, tb = route_trace(lambda: cb.Eval(toks, past))
            assert np.isnan(lb[5]) and np.isfinite(np.delete(lb, 5)).all() and np.abs(np.nan_to_num(lb)).max() > 0
            assert same(la, lb) and mapped(ta, tb) and tiles_only(ta, tb), (past, ta, tb)          # NaN by bit pattern
            for ra, rb in zip(cache_rows(ca, hp, 2, ctx, past, 89), cache_rows(cb, hp, 2, ctx, past, 89)):
                assert same(ra, rb), past
        sa, ta = route_trace(lambda: poisoned(ca).Score(toks, 0))
        sb, tb = route_trace(lambda: cb.Score(toks, 0))
        assert same(sa, sb) and mapped(ta, tb) and "k_expand_q4" not in families(ta) and families(ta).count("k_gemm_q4b3") == 4 * 2 + 1, (ta, tb)
    finally:
        ca.free(); cb.free(); A.free(); B.free()


# ---- 4. / 5. Score, both switches, toggles ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_twins(product):
    hp = make_hparams(**SHAPES["small"], ctx=160)
    A, B = twins(product, hp, seed=1234)
    yield hp, A, B
    A.free(); B.free()


def test_score_over_129_tokens(small_twins):
    hp, A, B = small_twins
    toks = [int(t) for t in np.random.default_rng(3).integers(0, hp.vocabSize, 129)]
    ca, cb = A.NewContext(160, 1), B.NewContext(160, 1)
    try:
        ca.SetQ4Tiles(True)
        sa, ta = route_trace(lambda: ca.Score(toks, 0))
        sb, tb = route_trace(lambda: cb.Score(toks, 0))
        assert same(sa, sb) and mapped(ta, tb) and tiles_only(ta, tb), (ta, tb)
        head_a, head_b = [e for e in ta if e.startswith("k_gemm_")][-1], [e for e in tb if e.startswith("k_gemm_")][-1]
        assert head_a.startswith("k_gemm_q4b3<") and head_b.startswith("k_gemm_q8b3<4>") and "k_expand_q4" not in families(ta), (ta, tb)
    finally:
        ca.free(); cb.free()


def test_both_switches_and_toggles(small_twins):
    hp, A, B = small_twins
    rng = np.random.default_rng(12)
    ca, cb = A.NewContext(160, 1), B.NewContext(160, 1)
    try:
        ca.SetQ4Stream(True)
        for n, on in ((88, True), (89, True), (89, False), (89, True)):
            ca.SetQ4Tiles(on)
            assert ca.q4_tiles is on and ca.q4_stream is True
            toks = [int(t) for t in rng.integers(0, hp.vocabSize, n)]
            la, ta = route_trace(lambda: poisoned(ca).Eval(toks, 0))
            lb, tb = route_trace(lambda: cb.Eval(toks, 0))
            fa = families(ta)
            assert same(la, lb), (n, on)
            assert ("k_stream_q4b" in fa) == (n == 88) and ("k_gemm_q4b3" in fa) == (n == 89 and on) == ("k_gemm_q8b3" not in fa and n == 89), (n, on, ta)
            assert ("k_expand_q4" in fa) == (not on), (n, on, ta)
            if on:
                assert mapped(ta, tb) or n == 88, (ta, tb)
    finally:
        ca.free(); cb.free()


# ---- 6. the switch ----------------------------------------------------------------------------------------------------------------------------------------------
def test_off_is_todays_trace(small_twins):
    hp, A, B = small_twins
    toks = [int(t) for t in np.random.default_rng(7).integers(0, hp.vocabSize, 89)]
    never, toggled = A.NewContext(160, 1), A.NewContext(160, 1)
    try:
        toggled.SetQ4Tiles(True)
        toggled.SetQ4Tiles(False)
        (l0, t0), (l1, t1) = route_trace(lambda: never.Eval(toks, 0)), route_trace(lambda: toggled.Eval(toks, 0))
        assert same(l0, l1) and t0 == t1 and "k_gemm_q8b3" in families(t0) and "k_gemm_q4b3" not in families(t0), (t0, t1)
        assert [k for k, _ in expand_runs(t0)] == [7] * hp.layersCount, t0            # the image in front of every layer
    finally:
        never.free(); toggled.free()


@pytest.mark.parametrize("kind", ["f32", "q8", "f16"])
def test_switch_does_nothing_for_other_weight_types(product, kind):
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=160)
    m = product.NewSyntheticModel(hp, 9)
    if kind == "q8":
        m.QuantizeQ8()
    elif kind == "f16":
        m.NarrowF16()
    toks = [int(t) for t in np.random.default_rng(90).integers(0, hp.vocabSize, 129)]
    res = []
    try:
        for on in (False, True):
            c = m.NewContext(160, 1)
            try:
                c.SetQ4Tiles(on)
                assert c.q4_tiles is on
                res.append(route_trace(lambda: c.Eval(toks, 0)))
            finally:
                c.free()
        (l0, t0), (l1, t1) = res
        assert same(l0, l1) and t0 == t1 and not set(families(t1)) & {"k_gemm_q4b3", "k_expand_q4"}, (t0, t1)
    finally:
        m.free()


CHILD = """
import sys
sys.path.insert(0, {root!r})
from llama_go_amd.mlapi import SHAPES, load_product, make_hparams
p = load_product()
m = p.NewSyntheticModel(make_hparams(**SHAPES["tiny"], ctx=16), 3)
c = m.NewContext(16, 1)
first = c.q4_tiles
c.SetQ4Tiles(not first)
print("q4_tiles", int(first), int(c.q4_tiles), int(c.q4_stream))
c.free(); m.free()
"""


@pytest.mark.parametrize("value,want", [("1", 1), ("0", 0), (None, 0)])
def test_environment_sets_the_initial_value_in_a_fresh_process(value, want):
    env = {k: v for k, v in os.environ.items() if k not in ("LLAMAHIP_Q4_TILES", "LLAMAHIP_ROUTE_FILE")}
    if value is not None:
        env["LLAMAHIP_Q4_TILES"] = value
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-4:] == ["q4_tiles", str(want), str(1 - want), "0"], r.stdout     # read at lh_ctx_create; the setter overrides it
