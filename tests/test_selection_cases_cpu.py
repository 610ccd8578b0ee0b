"""CPU (`-m "not gpu"`): the references of tests/test_gpu_selection.py are themselves held to each other on the very inputs the kernels see
(tests/selection_cases.py).  Greedy rows: the checker's llamago_Argmax == the restated rule == the id known by construction.  Sampler cases: the
checker's SampleTopPTopK == the numpy derivation of tests/sampler_ref.py - same candidates, bit-equal probabilities (NaN where +inf makes them
NaN), same token - so every case has one well-defined expected output and none needs to be left out."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selection_cases as sc   # noqa: E402


@pytest.fixture(scope="module")
def checker_argmax(oracle):
    f = oracle.lib.llamago_Argmax
    f.restype, f.argtypes = ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_uint32]
    return lambda x: int(f(x.ctypes.data, x.size))


@pytest.mark.parametrize("V", sc.ARGMAX_V)
def test_checker_argmax_equals_the_rule_on_every_row(checker_argmax, V):
    X, names, known = sc.argmax_rows(V)
    assert X.shape[0] >= (4 if V == 1 else 20)
    for x, name, want in zip(X, names, known):
        x = np.ascontiguousarray(x)
        r = sc.rule_argmax(x)
        if want is not None:
            assert r == want, (V, name)
        if V <= 4097:
            assert sc.rule_argmax_loop(x) == r, (V, name)
        assert checker_argmax(x) == r, (V, name)


def test_argmax_rows_cover_the_positions():
    """Every row's first three and last three ids carry a single maximum and take part in a tie; NaN rows exist at every size."""
    for V in sc.ARGMAX_V:
        _, names, _ = sc.argmax_rows(V)
        ends = {i for i in (0, 1, 2, V - 3, V - 2, V - 1) if 0 <= i < V}
        assert all(f"one maximum at {i}" in names for i in ends), V
        assert any(n.startswith("NaN") for n in names) and "all NaN" in names
        if V >= 65:
            tied = {int(t) for n in names if n.startswith("tie at") for t in n[8:-1].replace(" ", "").split(",") if t}
            assert {0, V - 1, 63, 64} <= tied, V
        if V > 16392:
            assert "tie at (8, 16392)" in names and "one maximum at 16384" in names


def test_sampler_case_lists_are_whole():
    g = sc.groups()
    assert set(g) == set(sc.GROUP_NAMES)
    for V in sc.SAMPLER_V:
        ks = {c.topK for c in g[f"grid V={V}"]}
        assert {k for k in sc.SAMPLER_K if k <= V} <= ks and (V > 1024 or V in ks)
        assert any(not c.ring for c in g[f"grid V={V}"]) and any(max(c.ring, default=0) >= V for c in g[f"grid V={V}"])
    assert len(g["mass ties K<=64"]) == len(g["mass ties K>64"]) == 32
    assert {c.topP for c in g["topP"]} >= {0.0, 1e-30, 0.999999, 1.0, 1.5} and sum(c.name == "topP never reached" for c in g["topP"]) == 2
    assert len(g["special values"]) == 32


@pytest.mark.parametrize("group", sc.GROUP_NAMES)
def test_checker_sampler_equals_numpy_on_every_case(oracle, group):
    ctx = oracle.NewContext(1)
    nan_rows = 0
    for i, c in enumerate(sc.groups()[group]):
        for draw in sc.DRAWS:
            tok, ids, probs = oracle.SampleTopPTopK(ctx, *c.args(), seed=sc.SEED, draw=draw, debug=True)
            rtok, rids, rprobs = sc.reference(group, i, draw)
            assert ids == rids, (c, draw)
            np.testing.assert_array_equal(probs, rprobs, err_msg=repr(c))      # bit-equal: both take libm's exp in f64 (NaN == NaN here)
            assert tok == rtok, (c, draw)
            assert oracle.SampleTopPTopK(ctx, *c.args(), seed=sc.SEED, draw=draw) == tok
            nan_rows += bool(np.isnan(rprobs).any())
    if group == "special values":
        assert nan_rows > 0     # the +inf rows are what makes equal_nan necessary
