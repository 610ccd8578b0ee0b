"""gpu: f16 models at 49..64 rows on k_stream_b9_h (lh_ctx_set_f16_planes; csrc/kernels_stream_b9_h.h, DESIGN 3k "Native planes kernel") - every
comparison is == on bytes.  Model A is narrowed (tests/test_gpu_f16.py's twins) and runs with the switch ON, B is its fp32 twin: A's logits and cache rows
are B's bytes and A's route trace is B's entry by entry, k_stream_b9_h<MAXT,NCT,NIMG,6>/sS for k_stream_b9<MAXT,NCT,NIMG,8>/sS (ring depth and product
count are no part of the sums), with no k_widen_f16 in front of a layer.  poisoned(): a read of a stale fp32 image would differ."""
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
from llama_go_amd.mlapi import Batch, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu
H = "k_stream_b9_h"


def norm(trace):
    """k_stream_b9[_h]<MAXT,NCT,NIMG,NPROD>/sS -> k_stream_b9<MAXT,NCT>/sS; widening passes and the decode GEMVs left out"""
    out = [re.sub(r"^k_stream_b9(?:_h)?<(\d+),(\d+),\d+,\d+>(/s\d+)$", r"k_stream_b9<\1,\2>\3", e) for e in trace]
    return [e for e in out if not e.startswith(("k_widen_f16", "k_gemv_"))]


def eval_pair(ca, cb, hp, layers, ctx, toks, past):
    la, ta = route_trace(lambda: poisoned(ca).Eval(toks, past))
    lb, tb = route_trace(lambda: cb.Eval(toks, past))
    assert np.isfinite(lb).all() and np.abs(lb).max() > 0 and same(la, lb), (len(toks), past)
    for which in (0, 1):
        for il in range(layers):
            off, n = (il * ctx + past) * hp.embdSize, len(toks) * hp.embdSize
            assert same(ca.CacheRead(which, off, n), cb.CacheRead(which, off, n)), (which, il)
    return ta, tb


def planes_checks(ta, tb, layers):
    """A's launches are B's, every k_stream_b9 of B a k_stream_b9_h of A; at most one widening pass, directly in front of an lm_head launch of another kernel"""
    fa, fb = families(ta), families(tb)
    assert norm(ta) == norm(tb), (ta, tb)
    assert fa.count(H) == fb.count("k_stream_b9") >= 4 * layers and "k_stream_b9" not in fa and H not in fb, (ta, tb)
    assert fa.count("k_widen_f16") <= 1, ta
    if "k_widen_f16" in fa:
        i = fa.index("k_widen_f16")
        assert i + 1 < len(fa) and H not in fa[i + 1:] and fa[:i].count(H) == 4 * layers, ta


def pair_of_contexts(product, shape, layers, ctx, prepare=None, **kw):
    hp = make_hparams(**dict(WP.SHAPES[shape], **kw), layers=layers, ctx=ctx)
    A, B = twins(product, hp, prepare=prepare)
    ca, cb = A.NewContext(ctx, 1), B.NewContext(ctx, 1)
    assert ca.f16_planes is False                      # off by default
    ca.SetF16Planes(True)
    assert ca.f16_planes is True and cb.f16_planes is False and ca.f16_stream is False and ca.f16_tiles is False
    seeded_cache((ca, cb), hp, layers, ctx)
    return hp, A, B, ca, cb


def free(*objs):
    for o in objs:
        o.free()


@pytest.fixture(scope="module")
def solo(product):
    made = {}
    yield lambda shape: made[shape] if shape in made else made.setdefault(shape, pair_of_contexts(product, shape, 2, 128))
    for hp, A, B, ca, cb in made.values():
        free(ca, cb, A, B)


# small: one tile per workgroup and workgroups without one, w1|w3 as pairs, 1 / 2 / 15 / 16 valid rows in the fourth column tile.
# 7Blayer: three tiles (the column split), six tiles as pairs, wo / w2 as K-split fours with the reduce pass feeding the next layer's planes.
@pytest.mark.parametrize("past", [0, 37])
@pytest.mark.parametrize("shape,n", [("small", 49), ("small", 50), ("small", 63), ("small", 64), ("7Blayer", 49), ("7Blayer", 64)])
def test_solo_evals_are_byte_equal_and_take_the_twins_launches(solo, shape, n, past):
    hp, _, _, ca, cb = solo(shape)
    toks = [int(t) for t in np.random.default_rng(100 * n + past).integers(0, hp.vocabSize, n)]
    ta, tb = eval_pair(ca, cb, hp, 2, 128, toks, past)
    planes_checks(ta, tb, 2)
    if shape == "7Blayer":
        hs = [e for e in ta if e.startswith(H)]
        assert hs[0].startswith(H + "<3,4,") and hs[2].startswith(H + "<6,4,") and hs[1].endswith("/s4") and hs[3].endswith("/s4"), ta


def on_batches(A, B, ctx, pods, fn):
    """fn(batch, poison) on a batch of A with the switch on and on a batch of B -> [(result, trace)] * 2"""
    res = []
    for m in (A, B):
        b = Batch(m, ctx, pods)
        try:
            assert b.batched
            if m is A:
                b.SetF16Planes(True)
            res.append(fn(b, m is A))
        finally:
            b.free()
    return res


def test_the_lm_head_reads_halves_in_one_launch_and_in_two(product):
    ctx, pods = 72, 64
    hp, A, B, ca, cb = pair_of_contexts(product, "7Blayer", 1, ctx, vocab=32000)
    rng = np.random.default_rng(21)
    try:
        ta, tb = eval_pair(ca, cb, hp, 1, ctx, [int(t) for t in rng.integers(0, hp.vocabSize, 64)], 0)   # one logits row: eight row tiles, one column tile
        planes_checks(ta, tb, 1)
        assert families(ta).count(H) == 5 and "k_widen_f16" not in families(ta) and [e for e in ta if e.startswith(H)][-1].startswith(H + "<8,1,"), ta
        prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 2)] for _ in range(pods)]

        def tick(b, poison):     # 64 logits rows: the output matrix as two half-vocabulary launches
            first = b.Prompt(prompts)
            return route_trace(lambda: poisoned(b, poison).Decode(first, [2] * pods, 1, want_logits=True))
        ((ia, la), ta), ((ib, lb), tb) = on_batches(A, B, ctx, pods, tick)
        fa = families(ta)
        assert ia == ib and same(la, lb) and norm(ta) == norm(tb), (ta, tb)
        assert "k_widen_f16" not in fa and "k_stream_b9" not in fa and fa.count(H) % 6 == 0 and fa.count(H) == families(tb).count("k_stream_b9") > 0, ta
    finally:
        free(ca, cb, A, B)


def test_ticks_follow_the_switch_and_are_captured_anew(product):
    hp = make_hparams(**WP.SHAPES["small"], layers=2, ctx=64)
    A, B = twins(product, hp, seed=1234)
    rng = np.random.default_rng(80)
    pods = 49
    prompts = [[int(t) for t in rng.integers(0, hp.vocabSize, 3)] for _ in range(pods)]
    ba, bb = Batch(A, 64, pods), Batch(B, 64, pods)
    try:
        first, past = poisoned(ba).Prompt(prompts), [3] * pods
        assert first == bb.Prompt(prompts)
        for seg, on in enumerate((True, True, False, False, True, True)):
            ba.SetF16Planes(on)
            assert ba.f16_planes is on
            (ia, la), ta = route_trace(lambda: poisoned(ba).Decode(first, past, 2, want_logits=True))
            ib, lb = bb.Decode(first, past, 2, want_logits=True)
            assert ia == ib and same(la, lb), seg
            fa = families(ta)
            if seg % 2 == 0:     # a changed switch (or the first tick): launched eagerly, then captured
                assert (H in fa) is on and ("k_stream_b9" in fa) is (not on) and (fa.count("k_widen_f16") == 0) is on, (seg, ta)
            else:                # the same value again: the captured tick is replayed
                assert not [f for f in fa if f.startswith("k_stream_")], (seg, ta)
            first, past = [r[-1] for r in ia], [p + 2 for p in past]
        firsts = [int(t) for t in rng.integers(0, hp.vocabSize, 16)]      # a speculative pass of 16 pods x 4 rows
        (ra, ta), (rb, tb) = on_batches(A, B, 64, 16, lambda b, poison: route_trace(lambda: poisoned(b, poison).DecodeLookup(firsts, [0] * 16, 6, 3, want_logits=True)))
        assert ra[0] == rb[0] and same(ra[1], rb[1]) and ra[2:] == rb[2:]
        assert H in families(ta) and "k_widen_f16" not in families(ta) and norm(ta) == norm(tb), (ta, tb)
    finally:
        free(ba, bb, A, B)


def test_subnormals_zeros_and_the_largest_halves(product):
    kw = WP.SHAPES["small"]
    d = kw["embd"]
    F = ((2 * (4 * d) // 3 + kw["mult"] - 1) // kw["mult"]) * kw["mult"]      # llama.go:210-211
    wq, w2 = value_matrix(d, d), all_values_matrix(d, F)     # the stream test's filling; the tile test's, which holds all 1023 subnormals with both signs
    for w in (wq, w2):
        assert int((np.abs(w) < 2.0 ** -14).sum()) > w.size // 2 and float(np.abs(w).max()) == 65504.0 and np.isfinite(w).all()
    assert len(np.unique(w2[(np.abs(w2) < 2.0 ** -14) & (w2 != 0)])) == 2 * 1023
    put = lambda m: (m.SetTensor("layers.0.attention.wq.weight", wq), m.SetTensor("layers.0.feed_forward.w2.weight", w2))   # noqa: E731
    hp, A, B, ca, cb = pair_of_contexts(product, "small", 2, 64, prepare=put)
    try:
        ta, tb = eval_pair(ca, cb, hp, 2, 64, [int(t) for t in np.random.default_rng(31).integers(0, hp.vocabSize, 49)], 0)
        planes_checks(ta, tb, 2)
    finally:
        free(ca, cb, A, B)


def test_a_refused_shape_keeps_its_route(product):
    hp, A, B, ca, cb = pair_of_contexts(product, "odd640", 2, 64)     # ff = 1712, no multiple of 128: Planes hands the Eval to Prefill
    try:
        toks = [int(t) for t in np.random.default_rng(5).integers(0, hp.vocabSize, 49)]
        t_on, tb = eval_pair(ca, cb, hp, 2, 64, toks, 0)
        ca.SetF16Planes(False)
        t_off, _ = eval_pair(ca, cb, hp, 2, 64, toks, 0)
        assert t_on == t_off and H not in families(t_on) and "k_stream_b9" not in families(tb), (t_on, t_off)
    finally:
        free(ca, cb, A, B)
