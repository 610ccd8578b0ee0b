"""Pins the bound of tests/weight_probe_ref.py before any GPU run: two plain float32 numpy evaluations of every case must stay inside it, and every
mutant of the float64 result must fall outside.

Cases: every (probe, shape, weight type) of the GPU test.  `small` and the odd shapes with all their rows (one reference covers every row count: the layer is
causal), the 7B layer with 24 rows and the 65B layer with 12: nothing in the bound depends on the row count but the row index T_j of the attention mean.
Block-int8 weights come from the numpy quantiser of the reference module, which tests/test_gpu_weight_probe.py holds bit for bit against the device's.

The float32 evaluations: the textbook order (one BLAS product per matrix), and every product in 32-wide K blocks summed one after the other, block-int8
matrices in the scale-factored form sum_b d_b (sum_k q_k x_k).  The worst error / bound ratio is printed; it is a report, not a cap.

The mutants (weight_probe_ref.MUTANTS): one 32-column block of one output row dropped; one block multiplied by its neighbour's scale (block-int8); w1 and
w3 exchanged for one row pair; gamma left out of one float4 of the norm; the residual missing / added twice in one element; row r of a 16-row tile taking
row r + 1's sums; one V row appended one cache position late; the middle bf16 plane of one activation row dropped.  Dropping only the LOWEST plane is 2^-16
relative per term and sits below a worst-case bound at these K: test_lowest_plane_is_below_the_bound states that instead of pretending otherwise."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as R   # noqa: E402

MODELS = [("small", "f32", None), ("small", "q8", None), ("odd640", "f32", None), ("odd640m32", "q8", None), ("7Blayer", "f32", 24), ("7Blayer", "q8", 24),
          ("65Blayer", "f32", 12)]
assert {(s, w) for s, w, _ in MODELS} == set(R.ROWS)
CASES = [(p, s, w, rows) for s, w, rows in MODELS for p in R.probes_of(s)]
IDS = [f"{p}-{s}-{w}" for p, s, w, _ in CASES]
REPORT = {}


@functools.lru_cache(maxsize=1)
def build_case(probe, shape, wtype, rows):
    """-> (X, device weights, {name: (q, d)} of the block-int8 matrices, reference)"""
    T = R.probe_tensors(probe, shape)
    Q = {n: R.quantize_q8(v) for n, v in T.items() if v.ndim == 2 and np.any(v)} if wtype == "q8" else {}
    W = {n: (Q[n][2] if n in Q else v) for n, v in T.items()}          # = R.as_device(T, wtype), quantised once
    X = R.inputs(shape, rows or R.total_rows(shape, wtype))
    return X, W, Q, R.reference(probe, W, X)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request):
    """module scope: pytest runs both tests of a case one after the other, so its reference is computed once"""
    return request.param, build_case(*request.param)


def test_case_matrix_is_the_issue_s():
    assert R.ff_size(1024, 256) == 2816 and R.ff_size(640, 8) == 1712 and R.ff_size(640, 32) == 1728 and R.ff_size(4096, 256) == 11008 and R.ff_size(8192, 256) == 22016
    assert R.ROWS["small", "f32"] == (1, 2, 4, 5, 8, 9, 16, 17, 48, 49, 64, 65, 128, 129, 192, 193) and R.ROWS["small", "q8"] == (1, 2, 4, 5, 16, 64, 65, 88, 89, 129)
    assert R.ROWS["odd640", "f32"] == (1, 3, 8, 9, 40) and R.ROWS["odd640m32", "q8"] == (1, 3, 8, 9, 40, 130)
    assert R.ROWS["7Blayer", "f32"] == (1, 4, 16, 64, 128) and R.ROWS["7Blayer", "q8"] == (1, 4, 16, 89) and R.ROWS["65Blayer", "f32"] == (5, 8)
    assert R.probes_of("65Blayer") == ("wv", "w13", "w2") and R.BOUND_C == 16 and R.U == 2.0 ** -24
    for (shape, wtype), rows in R.ROWS_PAST.items():       # one call per route family behind the cached rows
        assert {R.expected_route(shape, wtype, n)[0] for n in rows} == {R.expected_route(shape, wtype, n)[0] for n in R.ROWS[shape, wtype]}, (shape, wtype)


def test_probe_tensors_are_what_the_docstring_says():
    T = R.probe_tensors("w13", "odd640")
    d, F = 640, 1712
    assert T["w2"].shape == (d, F) and np.count_nonzero(T["w2"]) == F and all(T["w2"][j % d, j] == 1 for j in (0, 639, 640, 1711))
    T = R.probe_tensors("w2", "odd640")
    assert np.count_nonzero(T["w1"]) == F and T["w1"][700, 60] == np.float32(1.5) and T["w3"][1711, 1711 - 1280] == np.float32(-0.75)
    for p in R.PROBES:
        T = R.probe_tensors(p, "odd640")
        assert all(not np.any(T[n]) for n in R.ZERO[p]) and np.all(np.abs(T["g1"] - 1) < 0.6) and np.std(T["g1"]) > 0.05
    X = R.inputs("small", 200)
    rms = np.sqrt((X.astype(np.float64) ** 2).mean(axis=1))
    assert len(set(np.round(np.log2(rms)))) >= 6 and rms.min() > 0.1 and rms.max() < 10


def test_numpy_quantiser_states_the_rule():
    w = np.zeros((1, 96), dtype=np.float32)
    w[0, :32] = np.linspace(-2, 1, 32)
    w[0, 40], w[0, 70] = np.nan, 3.0
    q, d, deq = R.quantize_q8(w)
    assert d[0, 0] == np.float32(2) / np.float32(127) and q[0, 0] == -127 and q[0, 31] == np.rint(np.float32(1) / d[0, 0]) and deq[0, 0] == d[0, 0] * np.float32(-127)
    assert np.isnan(d[0, 1]) and not np.any(q[0, 32:64]) and np.all(np.isnan(deq[0, 32:64]))
    assert q[0, 70] == 127 and np.count_nonzero(q[0, 64:]) == 1 and deq[0, 70] == np.float32(d[0, 2] * np.float32(127))


def test_float32_evaluations_stay_inside(case):
    (probe, shape, wtype, rows), (X, W, Q, ref) = case
    assert np.all(np.isfinite(ref["out"])) and np.all(ref["bound"] > 0)
    r_text = R.ratio(R.f32_eval(probe, W, X), ref)
    r_blk = R.ratio(R.f32_eval(probe, W, X, blocked=True, Q=Q), ref)
    REPORT[probe, shape, wtype] = (r_text, r_blk)
    print(f"{probe} {shape} {wtype}: float32 error / bound: textbook {r_text:.4f}, 32-wide blocks{' scale-factored' if Q else ''} {r_blk:.4f}")
    assert r_text <= 1 and r_blk <= 1, (probe, shape, wtype, r_text, r_blk)


def test_every_mutant_falls_outside(case):
    (probe, shape, wtype, rows), (X, W, Q, ref) = case
    names = R.mutants_of(probe, wtype)
    assert set(names) <= set(R.MUTANTS)
    T = 8                                                  # the mutants strike rows 5 and 6: the layer is causal, the first eight rows hold them
    ref8 = dict(out=ref["out"][:T], bound=ref["bound"][:T])
    for name in names:
        y = R.reference(probe, W, X[:T], mutant=R.make_mutant(name, T))["out"]
        r = R.ratio(y, ref8)
        print(f"{probe} {shape} {wtype} {name}: error / bound {r:.3g}")
        assert r > 1, f"{probe} {shape} {wtype}: the mutant {name} stays inside the bound (error / bound {r:.3g})"


def test_every_mutant_is_applied_somewhere():
    seen = set()
    for p, s, w, _ in CASES:
        seen |= set(R.mutants_of(p, w))
    assert seen == set(R.MUTANTS)


def test_lowest_plane_is_below_the_bound():
    """What the bound does not see: the lowest bf16 plane of one activation row (2^-16 relative per term at most)."""
    X, W, Q, ref = build_case("wo", "small", "f32", None)
    f = np.float32
    xn = X[5].astype(np.float64)
    a = xn.astype(f)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(f)
    lo = (a - hi) - R.split3_mid(a).astype(f)
    assert np.all(np.abs(lo) <= np.abs(a) * 2.0 ** -15)
    # pushed through |R| the plane is K terms of at most 2^-15 |w z|, random in sign: about sqrt(K) 2^-16 of sum|w z|, against a bound of 16 u K = 2^-20 K
    K = X.shape[1]
    assert np.sqrt(K) * 2.0 ** -16 < R.BOUND_C * R.U * K


def test_zz_report():
    for (p, s, w), (a, b) in sorted(REPORT.items()):
        print(f"{p:5s} {s:10s} {w:4s} float32 error/bound: textbook {a:.4f}  blocked {b:.4f}")
