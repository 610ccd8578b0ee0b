"""not-gpu: the attention bound of tests/attention_ref.py judged on its own, before any kernel is measured against it.

  * every case of the matrix has the score regime it is named after (asserted on the float64 reference), and the two float32 evaluations of it - the
    textbook order and an online softmax over 32-key tiles - stay inside the bound;
  * the spread between those two float32 orders defines K_SPREAD, the factor of the comparative check;
  * a float32 tiled emulation with one planted mistake at a time leaves the bound in the cases named in CAUGHT_BY (and is inside it without the mistake).

No case is exempt from any assertion: ties are cases like the others."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R   # noqa: E402


@pytest.fixture(scope="module")
def evaluated():
    """name -> (case, E(textbook), E(tiled), bound ratios, rows the regime's property held for): the whole matrix, ideal weights."""
    res = {}
    for c in R.case_matrix():
        c.steps()
        X, W, rows = c.sequence(), c.weights(), c.checked_rows()
        ref = R.reference(X, W, c.H, rows)
        held = R.check_regime(c, ref, rows)
        a, b = R.f32_textbook(X, W, c.H, rows), R.f32_tiled(X, W, c.H, rows)
        res[c.name] = (c, R.case_error(a, ref), R.case_error(b, ref), R.bound_ratio(a, ref), R.bound_ratio(b, ref), held)
    return res


def test_every_regime_holds_and_float32_is_inside_the_bound(evaluated):
    """check_regime has asserted the property of every case already (the fixture); here: every regime is present on every route with rows it held for,
    and both float32 orders are inside the bound everywhere, by a wide margin (the bound is a worst case)."""
    by = {}
    for name, (c, ea, eb, ra, rb, held) in evaluated.items():
        assert ra <= 1 and rb <= 1, (name, ra, rb)
        key = (c.name.split("-")[0].rstrip("0123456789"), c.regime)
        by[key] = by.get(key, 0) + held
    for fam in ("dec", "rows", "split", "flash", "cut", "gemm"):     # (by name: the cut cases learn their route from the work list, compiled on first use)
        for regime in ("diffuse", "onehot", "diag", "tie", "ramp", "offset"):
            assert by.get((fam, regime), 0) > 0, (fam, regime, "no row of any case holds the regime's property")
    worst = max(max(v[3], v[4]) for v in evaluated.values())
    print(f"largest float32 error / bound over {len(evaluated)} cases: {worst:.4f}")
    assert worst < 0.25


def test_spread_of_two_float32_orders(evaluated):
    """K_SPREAD = 2 x the largest E(A) / E(B) between the two float32 orders, rounded up to a power of two (module docstring of attention_ref)."""
    name, spread = max(((n, max(v[1] / v[2], v[2] / v[1])) for n, v in evaluated.items()), key=lambda t: t[1])
    rule = 2 ** math.ceil(math.log2(2 * spread))
    print(f"largest spread {spread:.2f} in {name}: E(textbook) {evaluated[name][1]:.1f}, E(tiled) {evaluated[name][2]:.1f} -> rule gives {rule}, K_SPREAD = {R.K_SPREAD}")
    assert rule == R.K_SPREAD, (spread, rule, R.K_SPREAD)
    assert abs(spread - R.MEASURED_SPREAD) <= 0.25 * R.MEASURED_SPREAD, (spread, R.MEASURED_SPREAD)   # (the BLAS behind numpy's float32 products differs between hosts)


# mistake -> [(case, grouping of the emulation)]: where the mistake is caught.  mask_wide is judged on the rows whose next key is a real row of the
# sequence (the last row's would be the NaN of a cache row nobody wrote, which stale_included covers).
CAUGHT_BY = {
    "mask_wide": [("flash-n97-p31-ramp", "single"), ("split320-ramp", "chunk"), ("rows8-p40-onehot-past", "single")],
    "diag_dropped": [("dec-hd128-T129-onehot-diag", "single"), ("flash-n97-p31-onehot-diag", "pair"), ("dec-hd128-T129-diffuse", "single")],
    "tile_last_dropped": [("dec-hd128-T129-onehot-t127", "single"), ("flash-n97-p31-onehot-t31", "pair"), ("flash-n97-p31-tie-tiles", "pair")],
    "chunk_last_dropped": [("split320-onehot-c0last", "chunk"), ("dec-hd128-T129-onehot-t127", "chunk")],
    "rescale_skipped": [("flash-n97-p31-ramp", "single"), ("split320-ramp", "single"), ("dec-hd128-T129-onehot-prev", "single")],
    "merge_crossed": [("dec-hd128-T129-onehot-prev", "pair"), ("split320-ramp", "pair"), ("dec-hd128-T129-tie", "pair")],
    "part_sum_unscaled": [("split320-tie-chunks", "chunk"), ("split320-ramp", "chunk"), ("dec-hd128-T129-offset", "chunk")],
    "head_v_shifted": [("flash-n97-p31-diffuse", "single"), ("dec-hd128-T129-ramp", "single")],
    "stale_included": [("rows8-p40-onehot-past", "single"), ("dec-hd128-T129-ramp", "chunk")],
}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistake_leaves_the_bound(mistake):
    cases = {c.name: c for c in R.case_matrix()}
    assert set(CAUGHT_BY) == set(R.MISTAKES)
    for name, groups in CAUGHT_BY[mistake]:
        c = cases[name]
        X, W, rows = c.sequence(), c.weights(), c.checked_rows()
        if mistake == "mask_wide":
            rows = rows[rows < c.T - 1]
        ref = R.reference(X, W, c.H, rows)
        end = max(p + n for n, p in c.calls)
        clean = R.bound_ratio(R.f32_tiled(X, W, c.H, rows, call_end=end, groups=groups), ref)
        wrong = R.bound_ratio(R.f32_tiled(X, W, c.H, rows, call_end=end, groups=groups, mistake=mistake), ref)
        print(f"{mistake:20s} {name:32s} {groups:7s} clean {clean:.4f} of the bound, with the mistake {wrong:.3g}")
        assert clean <= 1, (name, groups, clean)
        assert wrong > 1, f"{mistake} in {name} ({groups}) stays inside the bound: {wrong}"


def test_reference_matches_a_direct_evaluation_of_one_row():
    """The vectorised reference against the formulas of the module docstring written out for a single row, element by element."""
    c = next(c for c in R.case_matrix() if c.name == "rows8-p40-tie")
    X, W = c.sequence().astype(np.float64), c.weights()
    H, hd, j = c.H, c.hd, 45
    xn = X / np.sqrt((X * X).mean(axis=1) + 1e-5)[:, None]
    a, b = W["wq"][0, 0], W["wk"][0, 0]
    out = np.zeros(c.d)
    for h in range(H):
        def rot(v, t):
            r = np.empty(hd)
            for i in range(hd // 2):
                ang = t * 10000.0 ** (-2.0 * i / hd)
                r[2 * i] = v[2 * i] * math.cos(ang) - v[2 * i + 1] * math.sin(ang)
                r[2 * i + 1] = v[2 * i] * math.sin(ang) + v[2 * i + 1] * math.cos(ang)
            return r
        qj = rot(a * xn[j, h * hd:(h + 1) * hd], j)
        s = np.array([qj @ rot(b * xn[t, h * hd:(h + 1) * hd], t) for t in range(j + 1)]) / math.sqrt(hd)
        p = np.exp(s - s.max())
        p /= p.sum()
        out[h * hd:(h + 1) * hd] = p @ xn[:j + 1, h * hd:(h + 1) * hd]
    ref = R.reference(c.sequence(), W, H, [j])
    assert np.allclose(ref["out"][0], X[j] + out, rtol=1e-12, atol=1e-15)
    assert np.all(ref["bound"] >= ref["floor"]) and np.all(ref["floor"] >= 0)   # (0 only in columns no key has a value in)
