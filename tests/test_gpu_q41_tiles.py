"""gpu: Q4_1 models on the bf16 tile GEMM of prompts beyond 128 rows (lh_ctx_set_q41_tiles; csrc/kernels_gemm_q41.h, DESIGN 3m "Native tile GEMM").

Model A is Q4_1 with the switch ON, model B its expanded fp32 twin (tests/test_gpu_q41.py's twins).  k_gemm_b9_q41 forms k_expand_q41's w' and feeds
k_gemm_b9's products in k_gemm_b9's order, so A's logits and cache rows are B's bytes and A's trace is B's entry by entry, k_gemm_b9_q41<1,8,4,1,NST>/sS
for k_gemm_b9<1,8,4,1,2>/sS with equal split counts; k_expand_q41 never stands in front of a native launch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as R   # noqa: E402
from test_gpu_f16 import seeded_cache   # noqa: E402
from test_gpu_f16_tiles import cache_rows   # noqa: E402
from test_gpu_q41 import Q41Probe, families, same, twins   # noqa: E402
from test_gpu_weight_probe import run_call   # noqa: E402
from llama_go_amd.mlapi import make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
N = "k_gemm_b9_q41"
SHAPE = R.SHAPES["7Blayer"]


def eval_pair(ca, cb, hp, layers, ctx, toks, past):
    """A (its weight images poisoned first: a launch that reads a slot this Eval did not fill computes NaN) and B: bytes of logits and cache rows -> traces"""
    ca.PoisonWeightImages()
    la, ta = route_trace(lambda: ca.Eval(toks, past))
    lb, tb = route_trace(lambda: cb.Eval(toks, past))
    assert np.isfinite(lb).all() and np.abs(lb).max() > 0
    assert same(la, lb), (len(toks), past, float(np.abs(la - lb).max()))
    for ra, rb in zip(cache_rows(ca, hp, layers, ctx, past, len(toks)), cache_rows(cb, hp, layers, ctx, past, len(toks))):
        assert same(ra, rb), (len(toks), past)
    return ta, tb


def native_checks(ta, tb, split=False):
    """A's trace is B's with the native kernel standing for k_gemm_b9; at most one expansion (the output matrix of the logits row), none in front of a native launch"""
    keep = lambda t: [re.sub(r"^k_gemm_b9_q41<1,8,4,1,\d+>", "k_gemm_b9<1,8,4,1,2>", e) for e in t if not e.startswith("k_expand_q41")]   # noqa: E731
    assert keep(ta) == tb, (ta, tb)
    fa, fb = families(ta), families(tb)
    assert fa.count(N) == fb.count("k_gemm_b9") > 0 and "k_gemm_b9" not in fa and N not in fb and fa.count("k_expand_q41") <= 1, (ta, tb)
    for i, e in enumerate(ta):
        if e.startswith("k_expand_q41"):
            rest = [x for x in ta[i + 1:] if x != "k_split3_rows"]          # (the logits row's k_gemv_sa launch is not traced: nothing may follow)
            assert not (rest and rest[0].startswith(N)), ta
    splits = {int(e.rsplit("/s", 1)[1]) for e in ta if e.startswith(N)}          # split: some launches split, some do not, and the reduce pass is there
    assert not split or (1 in splits and max(splits) > 1 and "k_splitk_reduce" in ta), ta


BIG_CTX = 264


@pytest.fixture(scope="module")
def big(product):
    hp = make_hparams(**SHAPE, layers=2, ctx=BIG_CTX)
    A, B = twins(product, hp)
    ca, cb = A.NewContext(BIG_CTX, 1), B.NewContext(BIG_CTX, 1)
    assert ca.q41_tiles is False                       # off by default
    ca.SetQ41Tiles(True)
    assert ca.q41_tiles is True and cb.q41_tiles is False
    seeded_cache((ca, cb), hp, 2, BIG_CTX)
    yield hp, ca, cb
    ca.free(); cb.free(); A.free(); B.free()


@pytest.mark.parametrize("n,past", [(193, 0), (193, 7), (257, 0), (257, 7)])
def test_prompts_are_the_twins_bytes_on_the_native_kernel(big, n, past):
    hp, ca, cb = big
    toks = [int(t) for t in np.random.default_rng(300 + n + past).integers(0, hp.vocabSize, n)]
    ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, toks, past)
    native_checks(ta, tb, split=n == 193)
    assert families(ta).count(N) >= 2 * 4, ta


def test_ragged_m_and_an_odd_first_slab(product):
    kw = dict(SHAPE, mult=32)
    ctx = 200
    hp = make_hparams(**kw, layers=1, ctx=ctx)
    F = R.ff_size(kw["embd"], kw["mult"])
    assert F == 10944 and F % 256 == 192 and F // 32 == 342
    A, B = twins(product, hp)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    ca.SetQ41Tiles(True)
    seeded_cache((ca, cb), hp, 1, ctx)
    try:
        toks = [int(t) for t in np.random.default_rng(41).integers(0, hp.vocabSize, 193)]
        ta, tb = eval_pair(ca, cb, hp, 1, ctx, toks, 0)
        native_checks(ta, tb, split=True)
        w2 = [e for e in ta if e.startswith(N)][3]                                     # wq|wk|wv, wo, w1|w3, w2
        s = int(w2.rsplit("/s", 1)[1])
        assert s > 1 and any((k * 342 // s) & 1 for k in range(s)), w2                  # a range of w2 begins at an odd slab
    finally:
        ca.free(); cb.free(); A.free(); B.free()


@pytest.mark.parametrize("probe", R.probes_of("7Blayer"))
def test_native_tiles_against_float64(product, monkeypatch, probe):
    """every element within the a-priori bound C u |W||z| of tests/weight_probe_ref.py (W holds the values w'), 193 rows at past 0, contexts made with
    LLAMAHIP_Q41_TILES=1; the reference side alone (f32_eval of the same inputs) is checked first."""
    monkeypatch.setenv("LLAMAHIP_Q41_TILES", "1")
    P = Q41Probe(product, "7Blayer", probe)
    try:
        layer = 2 if probe == "head" else 1
        names = {k: f"layers.{layer}.{v}" for k, v in R.TENSOR_NAMES.items()}
        if probe == "head":
            names.update(norm="norm.weight", output="output.weight")
        T = R.probe_tensors(probe, "7Blayer")
        W = {k: product.read(None, P.model.tensor(name)).reshape(T[k].shape) for k, name in names.items()}   # the values w' (Q41Probe keeps only its 11-row reference)
        P.X = R.inputs("7Blayer", 193)
        P.ref = R.reference(probe, W, P.X)
        rows = slice(192, 193) if probe == "head" else slice(0, 193)
        ref = dict(out=P.ref["out"][rows], bound=P.ref["bound"][rows])
        plain = R.ratio(R.f32_eval(probe, W, P.X)[rows], ref)
        y, trace = run_call(product, P, 193, 0)
        ratio = R.ratio(y, ref)
        print(f"{probe} 7Blayer n=193: error / bound {ratio:.4g} (plain float32: {plain:.4g}); {sorted(set(families(trace)))}")
        assert plain <= 1.0, (probe, plain)
        assert ratio <= 1.0, (probe, ratio)
        assert N in families(trace), trace
    finally:
        P.model.free()


def test_off_is_todays_route(big):
    hp, ca, cb = big
    ca.SetQ41Tiles(False)
    try:
        ta, tb = eval_pair(ca, cb, hp, 2, BIG_CTX, [int(t) for t in np.random.default_rng(7).integers(0, hp.vocabSize, 193)], 0)
    finally:
        ca.SetQ41Tiles(True)
    fa = families(ta)
    assert fa[0] == "k_expand_q41" and fa.count("k_expand_q41") >= 14 and N not in fa, ta
    assert [e for e in ta if not e.startswith("k_expand_q41")] == tb, (ta, tb)


@pytest.mark.parametrize("kind", ["f32", "q4"])
def test_switch_does_nothing_for_other_weight_types(product, kind):
    hp = make_hparams(**R.SHAPES["small"], layers=2, ctx=256)
    m = product.NewSyntheticModel(hp, 9)
    if kind == "q4":
        m.QuantizeQ4()
    toks = [int(t) for t in np.random.default_rng(90).integers(0, hp.vocabSize, 193)]
    res = []
    try:
        for on in (False, True):
            c = m.NewContext(256, 1)
            try:
                c.SetQ41Tiles(on)
                assert c.q41_tiles is on
                res.append(route_trace(lambda: c.Eval(toks, 0)))
            finally:
                c.free()
        (l0, t0), (l1, t1) = res
        assert same(l0, l1) and t0 == t1 and not set(families(t1)) & {N, "k_expand_q41"}, (t0, t1)
    finally:
        m.free()


@pytest.mark.parametrize("value", ["1", "0"])
def test_environment_sets_the_initial_value(value):
    code = ("from llama_go_amd.mlapi import load_product, make_hparams, SHAPES\n"
            "m = load_product().NewSyntheticModel(make_hparams(**SHAPES['tiny'], ctx=32), 3)\n"
            "print('initial', int(m.NewContext(32, 1).q41_tiles))\n")
    env = dict(os.environ, LLAMAHIP_Q41_TILES=value, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"initial {value}" in out.stdout, (out.stdout, out.stderr)
