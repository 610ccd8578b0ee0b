"""gpu: Q4_1 models on the weight-stream MFMA kernels (lh_ctx_set_q41_stream; csrc/kernels_stream_q41.h, DESIGN 3m "Native stream kernels") - every
comparison of results is == on bytes.

Model A is Q4_1 with the switch ON, model B its expanded fp32 twin (tests/test_gpu_q41.py's twins): A's logits and cache rows are B's bytes and A's trace
is B's entry by entry with the _q41 kernels for the plain ones (the ring depth, no part of the sums, ignored).  A's weight images are poisoned in front
of every call: a launch that reads a slot its own call did not fill computes NaN."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as R   # noqa: E402
from test_gpu_f16 import seeded_cache   # noqa: E402
from test_gpu_q41 import Q41Probe, families, same, twins   # noqa: E402
from test_gpu_q41_tiles import eval_pair   # noqa: E402
from test_gpu_weight_probe import run_call   # noqa: E402
from llama_go_amd.mlapi import SHAPES, Batch, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
NATIVE, PLAIN, CTX = ("k_stream_mm2_q41", "k_stream_dma_q41"), ("k_stream_mm2", "k_stream_dma"), 200


def norm(e):
    """a stream entry as the comparison sees it: _q41 -> plain, k_stream_dma's NIMG and PIPE dropped"""
    m = re.match(r"^(k_stream_(?:mm2|dma))(?:_q41)?<([0-9,]+)>(/s\d+)$", e)
    if not m:
        return e
    args = m.group(2).split(",")
    return f"{m.group(1)}<{','.join(args[:3] + args[5:])}>{m.group(3)}"


def native_checks(ta, tb, expansions=1):
    """A's trace without its expansions is B's under norm; native launches stand for ALL of B's stream launches; few expansions, none in front of a native one"""
    assert [norm(e) for e in ta if not e.startswith("k_expand_q41")] == [norm(e) for e in tb], (ta, tb)
    fa, fb = families(ta), families(tb)
    assert sum(fa.count(k) for k in NATIVE) == sum(fb.count(k) for k in PLAIN) > 0 and not set(fa) & set(PLAIN) and not set(fb) & set(NATIVE), (ta, tb)
    assert fa.count("k_expand_q41") <= expansions, ta
    assert not [i for i, f in enumerate(fa[:-1]) if f == "k_expand_q41" and fa[i + 1] in NATIVE], ta


@pytest.fixture(scope="module")
def pair(product):
    """pair(shape) -> (hp, context of A with the switch on, context of B), two layers each, made once per shape"""
    made = {}
    def get(shape):   # noqa: E306
        if shape not in made:
            hp = make_hparams(**R.SHAPES[shape], layers=2, ctx=CTX)
            A, B = twins(product, hp)
            ca, cb = A.NewContext(CTX, 1), B.NewContext(CTX, 1)
            assert ca.q41_stream is False and ca.SetQ41Stream(True) is None and ca.q41_stream is True and cb.q41_stream is False   # off by default
            seeded_cache((ca, cb), hp, 2, CTX)
            made[shape] = (hp, ca, cb, A, B)
        return made[shape][:3]
    yield get
    for _, ca, cb, A, B in made.values():
        ca.free(); cb.free(); A.free(); B.free()


# 9, 16: k_stream_mm2_q41, folded norm, KC 128 / 256 | 17..48: k_stream_dma_q41, KC 64 / 128, K-split pairs for wo / w2 | 65..128: five to eight column
# tiles (CS = 2 at eight) | 129, 192: two passes.  The 7B layer shape (six row tiles per workgroup, K = 11008) runs a few counts: 2 layers stand where 32 would
SOLO = ([("small", n, 0) for n in (9, 16, 17, 32, 33, 48, 65, 80, 81, 96, 97, 112, 113, 128, 129, 192)] + [("small", n, 7) for n in (9, 33, 128, 129)]
        + [("7Blayer", n, 0) for n in (9, 17, 33, 48, 65, 128)])


@pytest.mark.parametrize("shape,n,past", SOLO)
def test_solo_evals_are_the_twins_bytes_on_the_twins_kernels(pair, shape, n, past):
    hp, ca, cb = pair(shape)
    toks = [int(t) for t in np.random.default_rng(100 + n + past).integers(0, hp.vocabSize, n)]
    ta, tb = eval_pair(ca, cb, hp, 2, CTX, toks, past)
    native_checks(ta, tb)


@pytest.mark.parametrize("n", [17, 33])
def test_ragged_deal(product, n):
    """684 (w1, w3) tile pairs, which do not divide by the CU count: DMA instructions that span tiles of two matrices, clamped tile slots.  (w2's K = 10944
    is no multiple of 128: the twin launches the tile GEMM there, so w2 is expanded in front of it - two expansions with the logits row's.)"""
    kw = dict(R.SHAPES["7Blayer"], mult=32)
    hp = make_hparams(**kw, layers=1, ctx=64)
    assert (R.ff_size(kw["embd"], kw["mult"]) // 16) % 64 != 0
    A, B = twins(product, hp)
    ca, cb = A.NewContext(64, 1), B.NewContext(64, 1)
    ca.SetQ41Stream(True)
    seeded_cache((ca, cb), hp, 1, 64)
    try:
        toks = [int(t) for t in np.random.default_rng(n).integers(0, hp.vocabSize, n)]
        ta, tb = eval_pair(ca, cb, hp, 1, 64, toks, 5)
        native_checks(ta, tb, expansions=2)
        assert any(e.startswith("k_stream_dma_q41") for e in ta), ta
    finally:
        ca.free(); cb.free(); A.free(); B.free()


@pytest.fixture(scope="module")
def small_twins(product):
    """(hp, A, B) for batches.  Their prompts are 5 tokens per pod: up to 4 rows a Q4_1 model runs k_gemv_q41_rows, whose summation order is not the fp32
    twin's; from 5 rows on it runs the twin's kernels, so both batches hold the same cache rows when the ticks begin"""
    hp = make_hparams(**SHAPES["small"], ctx=64)
    A, B = twins(product, hp, seed=1234)
    yield hp, A, B
    A.free(); B.free()


@pytest.mark.parametrize("pods", [9, 16, 17, 32, 33, 48])
def test_batch_ticks_expand_nothing(small_twins, pods):
    hp, A, B = small_twins
    prompts = [[int(t) for t in np.random.default_rng(60 + pods).integers(0, hp.vocabSize, 5)] for _ in range(pods)]
    ba, bb = Batch(A, 64, pods), Batch(B, 64, pods)
    try:
        ba.SetQ41Stream(True)
        assert ba.batched and ba.q41_stream is True and bb.q41_stream is False
        first = ba.Prompt(prompts)
        assert first == bb.Prompt(prompts)
        ba.PoisonWeightImages()
        (ia, la), ta = route_trace(lambda: ba.Decode(first, [5] * pods, 4, want_logits=True))     # eager, captured, replayed
        (ib, lb), tb = route_trace(lambda: bb.Decode(first, [5] * pods, 4, want_logits=True))
        assert ia == ib and np.isfinite(lb).all() and same(la, lb)
        native_checks(ta, tb, expansions=0)            # the lm_head of pods rows is a stream launch too: no image is read at all
    finally:
        ba.free(); bb.free()


def test_toggle_between_ticks_captures_anew(small_twins):
    hp, A, B = small_twins
    pods = 9
    prompts = [[int(t) for t in np.random.default_rng(80).integers(0, hp.vocabSize, 5)] for _ in range(pods)]
    ba, bb = Batch(A, 64, pods), Batch(B, 64, pods)
    try:
        first = ba.Prompt(prompts)
        assert first == bb.Prompt(prompts)
        past = [5] * pods
        for seg, on in enumerate((False, True, False, False)):
            ba.SetQ41Stream(on)
            ba.PoisonWeightImages()
            (ia, la), ta = route_trace(lambda: ba.Decode(first, past, 3, want_logits=True))
            ib, lb = bb.Decode(first, past, 3, want_logits=True)
            assert ia == ib and same(la, lb), seg
            streams = [f for f in families(ta) if f.startswith("k_stream_")]
            if seg < 3:      # a changed switch: the tick runs eagerly once and is captured anew - its launches are traced twice
                assert streams and set(streams) <= set(NATIVE if on else PLAIN) and ("k_expand_q41" in families(ta)) != on, (seg, ta)
                assert len(streams) % 2 == 0 and streams[:len(streams) // 2] == streams[len(streams) // 2:], (seg, ta)
            else:            # the same value again: the captured tick is replayed
                assert not streams, (seg, ta)
            first, past = [r[-1] for r in ia], [p + 3 for p in past]
    finally:
        ba.free(); bb.free()


def test_off_is_todays_route(pair):
    hp, ca, cb = pair("small")
    ca.SetQ41Stream(False)
    try:
        ta, tb = eval_pair(ca, cb, hp, 2, CTX, [int(t) for t in np.random.default_rng(7).integers(0, hp.vocabSize, 17)], 0)
    finally:
        ca.SetQ41Stream(True)
    assert families(ta)[0] == "k_expand_q41" and families(ta).count("k_expand_q41") >= 14 and not set(families(ta)) & set(NATIVE), ta
    assert [e for e in ta if not e.startswith("k_expand_q41")] == tb, (ta, tb)


@pytest.mark.parametrize("kind", ["f32", "q4"])
def test_switch_does_nothing_for_other_weight_types(product, kind):
    hp = make_hparams(**R.SHAPES["small"], layers=2, ctx=64)
    m = product.NewSyntheticModel(hp, 9)
    if kind == "q4":
        m.QuantizeQ4()
    toks = [int(t) for t in np.random.default_rng(90).integers(0, hp.vocabSize, 33)]
    res = []
    try:
        for on in (False, True):
            c = m.NewContext(64, 1)
            try:
                c.SetQ41Stream(on)
                assert c.q41_stream is on
                res.append(route_trace(lambda: c.Eval(toks, 0)))
            finally:
                c.free()
        (l0, t0), (l1, t1) = res
        assert same(l0, l1) and t0 == t1 and not set(families(t1)) & set(NATIVE + ("k_expand_q41",)), (t0, t1)
    finally:
        m.free()


@pytest.mark.parametrize("probe", R.probes_of("7Blayer"))
def test_native_stream_against_float64(product, monkeypatch, probe):
    """every element within the a-priori bound of tests/weight_probe_ref.py, 33 rows, contexts made with LLAMAHIP_Q41_STREAM=1; the reference's own f32_eval first"""
    monkeypatch.setenv("LLAMAHIP_Q41_STREAM", "1")
    P = Q41Probe(product, "7Blayer", probe)
    try:
        layer = 2 if probe == "head" else 1
        names = {k: f"layers.{layer}.{v}" for k, v in R.TENSOR_NAMES.items()}
        if probe == "head":
            names.update(norm="norm.weight", output="output.weight")
        T = R.probe_tensors(probe, "7Blayer")
        W = {k: product.read(None, P.model.tensor(name)).reshape(T[k].shape) for k, name in names.items()}
        P.X = R.inputs("7Blayer", 33)
        P.ref = R.reference(probe, W, P.X)
        rows = slice(32, 33) if probe == "head" else slice(0, 33)
        ref = {k: P.ref[k][rows] for k in ("out", "bound")}
        plain = R.ratio(R.f32_eval(probe, W, P.X)[rows], ref)
        y, trace = run_call(product, P, 33, 0)
        ratio = R.ratio(y, ref)
        assert plain <= 1.0 and ratio <= 1.0 and set(families(trace)) & set(NATIVE), (probe, plain, ratio, trace)
    finally:
        P.model.free()


@pytest.mark.parametrize("value", ["1", "0"])
def test_environment_sets_the_initial_value(value):
    code = ("from llama_go_amd.mlapi import load_product, make_hparams, SHAPES\n"
            "m = load_product().NewSyntheticModel(make_hparams(**SHAPES['tiny'], ctx=32), 3)\n"
            "print('initial', int(m.NewContext(32, 1).q41_stream))\n")
    env = dict(os.environ, LLAMAHIP_Q41_STREAM=value, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"initial {value}" in out.stdout, (out.stdout, out.stderr)
