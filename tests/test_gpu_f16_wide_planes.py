"""gpu: f16 prompts of 65..128 rows on k_stream_b9w_h (lh_ctx_set_f16_planes + lh_ctx_set_wide_planes; csrc/kernels_stream_b9w_h.h, DESIGN 3k "Native wide
planes kernel") - every comparison is == on bytes.  Model A is narrowed f16 with both switches on and its weight images poisoned in front of every Eval; B
is its fp32 twin under SetWidePlanes, whose route tests/test_gpu_wide_planes.py holds to float64 bounds.  A's logits and cache rows are B's bytes and A's
trace is B's entry by entry, k_stream_b9w_h<MAXT,NCT,NIMG,6>/sS for k_stream_b9w<MAXT,NCT,NIMG,8>/sS (ring depth and product count are no part of the sums)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as WP         # noqa: E402
from test_gpu_f16 import families, poisoned, same, seeded_cache, twins   # noqa: E402
from test_gpu_f16_stream import value_matrix   # noqa: E402
from test_gpu_f16_tiles import all_values_matrix   # noqa: E402
from llama_go_amd.mlapi import make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
H, CTX = "k_stream_b9w_h", 176


def norm(trace):
    """k_stream_b9[w][_h]<MAXT,NCT,NIMG,NPROD>/sS -> k_stream_b9[w]<MAXT,NCT>/sS (the lm_head keeps k_stream_b9[_h] in passes of at most 64 rows)"""
    return [re.sub(r"^k_stream_b9(w?)(?:_h)?<(\d+),(\d+),\d+,\d+>(/s\d+)$", r"k_stream_b9\1<\2,\3>\4", e) for e in trace]


def pair_of_contexts(product, shape, prepare=None):
    hp = make_hparams(**WP.SHAPES[shape], layers=2, ctx=CTX)
    A, B = twins(product, hp, prepare=prepare)
    ca, cb = A.NewContext(CTX, 1), B.NewContext(CTX, 1)
    ca.SetF16Planes(True), ca.SetWidePlanes(True), cb.SetWidePlanes(True)
    assert ca.f16_planes and ca.wide_planes and cb.wide_planes and not cb.f16_planes and not ca.f16_stream
    seeded_cache((ca, cb), hp, 2, CTX)
    return hp, A, B, ca, cb


def check_pair(hp, ca, cb, n, past):
    """A == B in logits, written cache rows and (normalised) trace; A's layers ran on the new kernel alone, no widening pass anywhere; -> A's new launches"""
    toks = [int(t) for t in np.random.default_rng(100 * n + past).integers(0, hp.vocabSize, n)]
    la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
    lb, tb = route_trace(lambda: cb.Eval(toks, past))
    assert np.isfinite(lb).all() and np.abs(lb).max() > 0 and same(la, lb), (n, past)
    for which in (0, 1):
        for il in range(2):
            off, cnt = (il * CTX + past) * hp.embdSize, n * hp.embdSize
            assert same(ca.CacheRead(which, off, cnt), cb.CacheRead(which, off, cnt)), (which, il)
    fa = families(ta)
    assert norm(ta) == norm(tb) and H not in families(tb), (ta, tb)
    assert fa.count(H) == 8 and not {"k_stream_b9w", "k_stream_dma", "k_stream_dma_h", "k_widen_f16"} & set(fa), ta
    return [e for e in ta if e.startswith(H + "<")]


@pytest.fixture(scope="module")
def solo(product):
    made = {}
    yield lambda shape: made[shape] if shape in made else made.setdefault(shape, pair_of_contexts(product, shape))
    for hp, A, B, ca, cb in made.values():
        for o in (ca, cb, A, B):
            o.free()


# small: one tile per workgroup and workgroups without one, w1|w3 as pairs, 1 and 16 valid rows in the last of five to eight column tiles.
# 7Blayer: three tiles, six tiles as pairs, wo / w2 as K-split fours whose reduce pass feeds the next planes.
@pytest.mark.parametrize("shape,n,past", [("small", n, 0) for n in (65, 80, 81, 96, 97, 112, 113, 128)] + [("small", 97, 37), ("7Blayer", 65, 0), ("7Blayer", 128, 37)])
def test_evals_are_byte_equal_and_take_the_twins_launches(solo, shape, n, past):
    hp, _, _, ca, cb = solo(shape)
    hs = check_pair(hp, ca, cb, n, past)
    if shape == "7Blayer":
        nct = (n + 15) // 16
        assert hs[0].startswith(f"{H}<3,{nct},") and hs[2].startswith(f"{H}<6,{nct},") and hs[1].endswith("/s4") and hs[3].endswith("/s4"), hs


def test_subnormals_zeros_and_the_largest_halves(product):
    kw = WP.SHAPES["small"]
    d = kw["embd"]
    F = ((2 * (4 * d) // 3 + kw["mult"] - 1) // kw["mult"]) * kw["mult"]      # llama.go:210-211
    wq, w2 = value_matrix(d, d), all_values_matrix(d, F)     # the stream test's filling; the tile test's, which holds all 1023 subnormals with both signs
    for w in (wq, w2):
        assert int((np.abs(w) < 2.0 ** -14).sum()) > w.size // 2 and float(np.abs(w).max()) == 65504.0 and np.isfinite(w).all()
    assert len(np.unique(w2[(np.abs(w2) < 2.0 ** -14) & (w2 != 0)])) == 2 * 1023
    put = lambda m: (m.SetTensor("layers.0.attention.wq.weight", wq), m.SetTensor("layers.0.feed_forward.w2.weight", w2))   # noqa: E731
    hp, A, B, ca, cb = pair_of_contexts(product, "small", prepare=put)
    try:
        check_pair(hp, ca, cb, 65, 0)
    finally:
        for o in (ca, cb, A, B):
            o.free()


@pytest.fixture(scope="module")
def four(product):
    """per shape: one f16 model and four contexts - no switch, f16 planes only, wide planes only, both"""
    made = {}

    def get(shape):
        if shape not in made:
            hp = make_hparams(**WP.SHAPES[shape], layers=2, ctx=136)
            m = product.NewSyntheticModel(hp, 1234)
            assert m.NarrowF16() > 0 and m.weight_type == 1
            cs = [m.NewContext(136, 1) for _ in range(4)]
            cs[1].SetF16Planes(True), cs[2].SetWidePlanes(True), cs[3].SetF16Planes(True), cs[3].SetWidePlanes(True)
            made[shape] = (hp, m, cs)
        return made[shape]
    yield get
    for hp, m, cs in made.values():
        for o in cs + [m]:
            o.free()


@pytest.mark.parametrize("shape,n", [("small", 64), ("small", 65), ("small", 128), ("small", 129), ("odd640", 65)])   # odd640: ff no multiple of 128, refused
def test_the_switch_pair_moves_only_its_band(four, shape, n):
    hp, _, cs = four(shape)
    toks = [int(t) for t in np.random.default_rng(n).integers(0, hp.vocabSize, n)]
    (l0, t0), (lp, tp), (lw, tw), (lb, tb) = [route_trace(lambda c=c: c.Eval(toks, 0).copy()) for c in cs]
    assert tw == t0 and same(lw, l0), (tw, t0)
    if n != 64:
        assert tp == t0 and same(lp, l0), (tp, t0)
    if n == 64:
        assert tb == tp and same(lb, lp), (tb, tp)
    elif n == 129 or shape == "odd640":
        assert tb == t0 and same(lb, l0) and H not in families(tb), (tb, t0)
    else:
        assert families(tb).count(H) == 8 and H not in families(t0) + families(tp) + families(tw), tb
