"""gpu: fp32 prompts of 65..128 rows in ONE pass on k_stream_b9w (lh_ctx_set_wide_planes; csrc/kernels_stream_b9w.h).
Per launch against the float64 references the other routes are held to (tests/weight_probe_ref.py with BOUND_C = 16 as it stands; tests/cache_probe_ref.py
for K, V and q), the route trace with the switch on and off, byte reproducibility, and the last-row logits against the route the switch replaces."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_probe_ref as CP            # noqa: E402
import weight_probe_ref as WP           # noqa: E402
import test_gpu_cache_probe as TC       # noqa: E402
import test_gpu_weight_probe as TW      # noqa: E402
from test_gpu_ops import close          # noqa: E402
from llama_go_amd.mlapi import make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
NEW, OLD = "k_stream_b9w", "k_stream_dma"
# small: one tile per workgroup, workgroups without a tile, w1|w3 as pairs; 1 and 16 valid rows in the last of five, six, seven and eight column tiles.
# 7Blayer: three tiles on wq|wk|wv, six as pairs, wo / w2 as K-split fours whose reduce pass writes the next planes.  One row count each behind WP.PAST rows.
CALLS = [("small", n, 0) for n in (65, 80, 81, 96, 97, 112, 113, 127, 128)] + [("small", 97, WP.PAST), ("7Blayer", 65, 0), ("7Blayer", 128, 0), ("7Blayer", 128, WP.PAST)]


def layer_launches(trace, layers=1):
    """the stream launches of a trace whose layers ran on the new kernel: 4 per layer, none of the old kernel; -> them"""
    new = [e for e in trace if e.startswith(NEW + "<")]
    assert len(new) == 4 * layers and not [e for e in trace if e.startswith(OLD)], trace
    return new


@pytest.fixture(scope="module")
def probe_of(product):
    alive = {}

    def get(shape, probe):           # one probe model at a time (the cases come probe by probe)
        if (shape, probe) not in alive:
            for k in list(alive):
                alive.pop(k).free()
            alive[shape, probe] = TW.Probe(product, shape, "f32", probe)
        return alive[shape, probe]
    yield get
    for k in list(alive):
        alive.pop(k).free()


@pytest.mark.parametrize("shape,n,past", CALLS)
@pytest.mark.parametrize("probe", WP.PROBES)
def test_every_launch_inside_the_float64_bound(product, probe_of, monkeypatch, probe, shape, n, past):
    monkeypatch.setenv("LLAMAHIP_WIDE_PLANES", "1")          # read by lh_ctx_create: the context TW.run_call makes has the switch on
    P = probe_of(shape, probe)
    y, trace = TW.run_call(product, P, n, past)
    new = layer_launches(trace)
    if shape == "7Blayer":
        nct = (n + 15) // 16
        assert new[0].startswith(f"{NEW}<3,{nct},") and new[2].startswith(f"{NEW}<6,{nct},") and new[1].endswith("/s4") and new[3].endswith("/s4"), trace
    rows = slice(past + n - 1, past + n) if probe == "head" else slice(past, past + n)
    ref = dict(out=P.ref["out"][rows], bound=P.ref["bound"][rows])
    print(f"{probe} {shape} n={n} past={past}: error / bound {WP.ratio(y, ref):.4g}")
    err = np.abs(y.astype(np.float64) - ref["out"])
    assert np.all(err <= ref["bound"]), f"{np.count_nonzero(~(err <= ref['bound']))} elements outside the bound, worst error / bound {WP.ratio(y, ref):.3g}"


@pytest.fixture(scope="module")
def cache_models(product):
    made = {}

    def get(probe, ctx):
        if probe not in made:
            made[probe] = TC.ProbeModel(product, "small", "f32", probe, ctx)
            for c in made[probe].ctxs:
                assert c.wide_planes is False                 # off by default
                c.SetWidePlanes(True)
                assert c.wide_planes is True
        return made[probe]
    yield get
    for m in made.values():
        m.free()


@pytest.mark.parametrize("past", [0, 37])
@pytest.mark.parametrize("n", [65, 97, 128])
def test_cache_rows_and_q_inside_the_float64_bound(cache_models, n, past):
    """K and V: two layers, every element of the written rows inside cache_probe_ref's bound, no float outside them changed.  q: the reference needs
    hd = 128 host-written keys in front (cache_probe_ref.q_reference asserts P >= hd), so its calls sit at past + 128."""
    M = cache_models("kv-dense", CP.CTX)
    _, K, V, trace, x = TC.run_call(M, n, past)
    layer_launches(trace, 2)
    pos = past + np.arange(n)
    chk = CP.check_cache(K, V, CP.kv_reference(M.W, x, pos, M.H), pos)
    print(f"kv n={n} past={past}: K error / bound {chk['rK']:.4g}, V {chk['rV']:.4g}, stray {chk['stray']}")
    assert chk["rK"] <= 1 and chk["rV"] <= 1 and chk["stray"] == 0, chk
    Q = cache_models("q", TC.Q_CTX)
    P = past + CP.head_dim("small")
    base = []
    for kv, rows in enumerate(CP.q_prefill(Q.H, CP.head_dim("small"), P)):
        img = TC.sentinel(kv, TC.Q_CTX * Q.d).copy().reshape(1, TC.Q_CTX, Q.d)
        img[0, :P] = rows
        base.append(img)
    y, _, _, trace, x = TC.run_call(Q, n, P, base=base)
    layer_launches(trace)
    ref = CP.q_reference(Q.W[0], x, P, Q.H)
    print(f"q n={n} P={P}: error / bound {CP.ratio(y, ref):.4g}")
    assert np.all(np.abs(y.astype(np.float64) - ref["out"]) <= ref["bound"]), CP.ratio(y, ref)


@pytest.fixture(scope="module")
def model2(product):
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=256)
    m = product.NewSyntheticModel(hp, 1234)
    on, off = m.NewContext(256, 1), m.NewContext(256, 1)
    on.SetWidePlanes(True)
    yield hp, on, off
    for o in (on, off, m):
        o.free()


def tokens(hp, n):
    return [int(t) for t in np.random.default_rng(n).integers(0, hp.vocabSize, n)]


@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_the_switch_moves_65_to_128_rows_and_nothing_else(model2, n):
    """Switch on: 65..128 rows launch the new kernel in every layer, the old one nowhere, and the last-row logits agree with the route it replaces inside
    tests/test_gpu_ops.py's fp32 route tolerance (max |delta| <= 1e-5 max |y|).  64 and 129 rows, or the switch off: the trace of a context that never had
    the switch, entry by entry, and the same bytes."""
    hp, on, off = model2
    la, ta = route_trace(lambda: on.Eval(tokens(hp, n), 0).copy())
    lb, tb = route_trace(lambda: off.Eval(tokens(hp, n), 0).copy())
    assert not [e for e in tb if e.startswith(NEW)], tb
    if 65 <= n <= 128:
        layer_launches(ta, 2)
        print(f"n={n}: max |on - off| / max |off| = {float(np.abs(la - lb).max()) / float(np.abs(lb).max()):.3g}")
        assert [e for e in tb if e.startswith(OLD)] and np.isfinite(lb).all() and np.abs(lb).max() > 0 and close(la, lb, 1e-5), tb
    else:
        assert ta == tb and la.tobytes() == lb.tobytes(), (ta, tb)


def test_the_same_eval_twice_leaves_the_same_bytes(model2):
    hp, on, _ = model2
    toks, got = tokens(hp, 100), []
    for _ in range(2):
        logits = on.Eval(toks, 0).copy()
        got.append((logits.tobytes(), [on.CacheRead(kv, il * 256 * hp.embdSize, 100 * hp.embdSize).tobytes() for kv in (0, 1) for il in (0, 1)]))
    assert got[0] == got[1]
