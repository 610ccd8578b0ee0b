"""Pins the bound of tests/cache_probe_ref.py before any GPU run: two plain float32 numpy evaluations of every case stay inside it (kv-sparse: inside HALF of
it - the bound has room over rounding noise and is not slack), and every mutant of the float64 result falls outside in at least one element of at least one
case - judged by the very check the GPU test applies to a cache it read back (check_cache: the bound on K, the bound on V, the sentinel everywhere else).

Cases: the shapes of at most 1024 columns with head sizes 128 (small, odd640), 64, 32 and 16, fp32 and block-int8 (the numpy quantiser of
tests/weight_probe_ref.py, held bit for bit against the device's by tests/test_gpu_weight_probe.py), a two-layer stage, calls of 9 rows at past = 0, 1, 7 and
ctx - 9 (ctx = 256; `small` also at ctx = 2048).  The q probe at past = hd and past = ctx - 9.  A batch of three pods for the mutant that only a batch has.

The mutants (cache_probe_ref.MUTANTS): position + 1 on K only / on q only; the row index used without `past`; pair i takes pair i + 1's angle; only the
lowest-frequency pair takes its neighbour's; the sign of sin flipped; the partner swapped; the head wrap e mod 2 hd; V rotated; the K and V slices exchanged;
cache row pos + 1; slot 0 written by both layers; the second half of a two-pass call rotated from `past`; pod i's rows at pod 0's position; one row more than
asked for.  test_each_check_is_needed states which mutants only ONE of the checks sees."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_probe_ref as R   # noqa: E402

N_ROWS = 9
MODELS = [("small", "f32", 256), ("small", "q8", 256), ("small", "f32", 2048), ("odd640", "f32", 256), ("hd64", "f32", 256), ("hd64", "q8", 256),
          ("hd32", "f32", 256), ("hd32", "q8", 256), ("hd16", "f32", 256), ("hd16", "q8", 256)]
IDS = [f"{s}-{w}-ctx{c}" for s, w, c in MODELS]
REPORT = {}
KILLS = {}       # mutant -> set of the checks that saw it somewhere: "K", "V", "sentinel", "q", "batch"


def pasts(ctx):
    return (0, 1, 7, ctx - N_ROWS)


@functools.lru_cache(maxsize=2)
def build(probe, shape, wtype):
    """-> (X, [device weights per layer], [{name: (q, d)} per layer])"""
    S = 1 if probe == "q" else 2
    Ts = [R.probe_tensors(probe, shape, L) for L in range(S)]
    Qs = [({n: R.quantize_q8(v) for n, v in T.items() if v.ndim == 2 and np.any(v)} if wtype == "q8" else {}) for T in Ts]
    Ws = [{n: (Q[n][2] if n in Q else v) for n, v in T.items()} for T, Q in zip(Ts, Qs)]
    return R.inputs(shape, 64), Ws, Qs


def test_case_matrix_is_the_issue_s():
    assert R.HD_SHAPES == dict(hd64=dict(vocab=2048, embd=1024, mult=256, heads=16), hd32=dict(vocab=2048, embd=1024, mult=256, heads=32),
                               hd16=dict(vocab=515, embd=640, mult=32, heads=40))
    assert [R.head_dim(s) for s in ("small", "hd64", "hd32", "hd16", "7Blayer", "65Blayer")] == [128, 64, 32, 16, 128, 128]
    assert R.HD_ROWS == (1, 3, 8, 9, 16, 17, 64, 65, 129, 193) and R.LONG_ROWS == (1, 4, 16, 64, 129) and R.LONG_CTX == 2048
    assert R.U == 2.0 ** -24 and R.BOUND_C == 16 and R.delta_common(1024) == 12 * R.U
    for s in ("hd64", "hd32"):
        for w in ("f32", "q8"):
            assert all(R.expected_route(s, w, n) == R.expected_route("small", w, n) for n in R.HD_ROWS)
    assert {R.expected_route("hd16", "q8", n)[0] for n in R.HD_ROWS} == {"Step", "Rows", "Q8Steps"}
    assert len({R.expected_route("hd16", "f32", n)[0] for n in R.HD_ROWS}) == 5


def test_probe_tensors_are_what_the_docstring_says():
    d = 640
    T0, T1 = R.probe_tensors("kv-sparse", "hd16", 0), R.probe_tensors("kv-sparse", "hd16", 1)
    for T in (T0, T1):
        assert np.count_nonzero(T["wk"]) == d and np.count_nonzero(T["wv"]) == d and not np.any(T["wq"]) and not np.any(T["wo"])
        assert not (np.any(T["w1"]) or np.any(T["w2"]) or np.any(T["w3"]))
    assert T0["wk"][0, 1] == 0.25 and T0["wk"][4, 5] == 4 and T0["wk"][639, 0] == 2.0 ** ((639 % 5) - 2) and T0["wv"][0, 3] == 0.5 and T0["wv"][638, 1] == 2.0 ** ((638 % 3) - 1)
    assert T1["wk"][0, 1] == 0.5 and not np.array_equal(T0["g1"], T1["g1"]) and np.std(T0["g1"]) > 0.05
    Tq = R.probe_tensors("q", "hd16")
    assert np.array_equal(Tq["wo"], 64 * np.eye(d, dtype=np.float32)) and not np.any(Tq["wk"]) and not np.any(Tq["wv"]) and np.count_nonzero(Tq["wq"]) == d * d
    Td0, Td1 = R.probe_tensors("kv-dense", "hd16", 0), R.probe_tensors("kv-dense", "hd16", 1)
    assert not np.array_equal(Td0["wk"], Td1["wk"]) and abs(np.std(Td0["wv"]) * np.sqrt(d) - 1) < 0.05
    K, V = R.q_prefill(40, 16, 20)
    assert K.shape == (20, d) and K[3, 16 * 7 + 3] == 8 and V[3, 16 * 7 + 3] == 1 and np.count_nonzero(K) == 16 * 40 and not np.any(K[16:]) and not np.any(V[16:])
    s0, s1 = R.sentinel(0, 100000), R.sentinel(1, 100000)
    assert np.all(np.isfinite(s0)) and s0.min() >= 1024 and len(np.unique(s0)) == 8191 and not np.any(s0 == s1) and np.all(s0[:-1] != s0[1:])


def kv_call(shape, wtype, probe, ctx, past, mut=None, f32=None):
    """One call of N_ROWS rows at `past` -> (check_cache of the images the evaluation leaves, the clean reference)."""
    X, Ws, Qs = build(probe, shape, wtype)
    H = R.SHAPES[shape]["heads"]
    d = X.shape[1]
    rows = R.call_rows(len(X), N_ROWS, past)
    pos = past + np.arange(N_ROWS)
    ref = R.kv_reference(Ws, X[rows], pos, H)
    res = R.kv_f32(Ws, X[rows], pos, H, order=f32, Q=Qs) if f32 is not None else R.kv_reference(Ws, X[rows], pos, H, mut=mut)
    K_img, V_img = R.cache_images(res, 2, ctx, d)
    return R.check_cache(K_img, V_img, ref, pos), ref


@pytest.mark.parametrize("shape,wtype,ctx", MODELS, ids=IDS)
@pytest.mark.parametrize("probe", R.KV_PROBES)
def test_float32_evaluations_stay_inside(probe, shape, wtype, ctx):
    worst = [0.0, 0.0]
    for past in pasts(ctx):
        for order in (0, 1):
            chk, ref = kv_call(shape, wtype, probe, ctx, past, f32=order)
            assert np.all(ref["bK"] > 0) and np.all(ref["bV"] > 0) and np.all(np.isfinite(ref["K"]))
            assert chk["stray"] == 0
            worst[order] = max(worst[order], chk["rK"], chk["rV"])
    REPORT[probe, shape, wtype, ctx] = tuple(worst)
    print(f"{probe} {shape} {wtype} ctx={ctx}: float32 error / bound: textbook {worst[0]:.4f}, other order {worst[1]:.4f}")
    cap = 0.5 if probe == "kv-sparse" else 1.0
    assert max(worst) <= cap, (probe, shape, wtype, ctx, worst)


@pytest.mark.parametrize("shape,wtype,ctx", MODELS, ids=IDS)
def test_every_kv_mutant_falls_outside(shape, wtype, ctx):
    """On kv-sparse, over the four positions of the model: the worst error / bound of each mutant, and which checks saw it."""
    for mut in R.KV_MUTANTS:
        rK = rV = 0.0
        stray = 0
        for past in pasts(ctx):
            chk, _ = kv_call(shape, wtype, "kv-sparse", ctx, past, mut=mut)
            rK, rV, stray = max(rK, chk["rK"]), max(rV, chk["rV"]), stray + chk["stray"]
        seen = {n for n, hit in (("K", rK > 1), ("V", rV > 1), ("sentinel", stray > 0)) if hit}
        KILLS.setdefault(mut, []).append(seen)
        print(f"kv-sparse {shape} {wtype} ctx={ctx} {mut}: K error / bound {rK:.3g}, V {rV:.3g}, stray floats {stray}")
        assert seen, f"{shape} {wtype} ctx={ctx}: the mutant {mut} passes every check"


@pytest.mark.parametrize("shape,wtype,ctx", MODELS, ids=IDS)
def test_q_probe_float32_inside_mutants_outside_and_not_blind(shape, wtype, ctx):
    X, Ws, Qs = build("q", shape, wtype)
    H = R.SHAPES[shape]["heads"]
    hd = R.head_dim(shape)
    worst = [0.0, 0.0]
    killed = {m: 0.0 for m in R.Q_MUTANTS}
    for P in (hd, ctx - N_ROWS):
        x = X[R.call_rows(len(X), N_ROWS, P)]
        ref = R.q_reference(Ws[0], x, P, H)
        assert np.all(ref["bound"] > 0) and np.all(ref["attn"] > 0)
        for order in (0, 1):
            worst[order] = max(worst[order], R.ratio(R.q_f32(Ws[0], x, P, H, order, Qs[0]), ref))
        # the probe must see: the bound of nearly every element far below the term that carries q
        sharp = np.mean(ref["bound"] < 2.0 ** -12 * ref["attn"])
        print(f"q {shape} {wtype} ctx={ctx} P={P}: {100 * sharp:.1f} % of the elements have a bound below 2^-12 of their attention term")
        assert sharp >= 0.95, (shape, wtype, ctx, P, sharp)
        for mut in R.Q_MUTANTS:
            killed[mut] = max(killed[mut], R.ratio(R.q_reference(Ws[0], x, P, H, mut=mut)["out"], ref))
    print(f"q {shape} {wtype} ctx={ctx}: float32 error / bound: textbook {worst[0]:.4f}, other order {worst[1]:.4f}")
    REPORT["q", shape, wtype, ctx] = tuple(worst)
    assert max(worst) <= 1, (shape, wtype, ctx, worst)
    for mut, r in killed.items():
        print(f"q {shape} {wtype} ctx={ctx} {mut}: error / bound {r:.3g}")
        if mut not in R.KV_MUTANTS:                                # (the others are judged on the cache, where they show sharper)
            KILLS.setdefault(mut, []).append({"q"} if r > 1 else set())
        assert r > 1, f"q {shape} {wtype} ctx={ctx}: the mutant {mut} stays inside the bound (error / bound {r:.3g})"


def batch_call(shape, wtype, mut=None):
    """Three pods, each its own rows at its own position of its own cache -> per pod (check_cache, stray)."""
    X, Ws, _ = build("kv-sparse", shape, wtype)
    H, d, ctx = R.SHAPES[shape]["heads"], X.shape[1], 64
    feeds = [(np.array([3]), 7), (np.array([9, 10, 11, 12, 13]), 1), (np.array([20]), 40)]
    out = []
    for tok, past in feeds:
        pos = past + np.arange(len(tok))
        ref = R.kv_reference(Ws, X[tok], pos, H)
        got_pos = feeds[0][1] + np.arange(len(tok)) if mut == "pod0_pos" else pos
        res = R.kv_reference(Ws, X[tok], got_pos, H)
        out.append(R.check_cache(*R.cache_images(res, 2, ctx, d), ref, pos))
    return out


@pytest.mark.parametrize("shape,wtype", [("small", "f32"), ("small", "q8"), ("hd32", "f32")])
def test_batch_mutant_falls_outside(shape, wtype):
    clean = batch_call(shape, wtype)
    assert all(c["rK"] <= 0.5 and c["rV"] <= 0.5 and c["stray"] == 0 for c in clean)        # (the float64 rows rounded to float32: half an ulp)
    bad = batch_call(shape, wtype, "pod0_pos")
    print(f"batch {shape} {wtype} pod0_pos: per pod K error / bound {[round(c['rK'], 1) for c in bad]}, stray floats {[c['stray'] for c in bad]}")
    assert bad[0]["rK"] <= 0.5 and bad[0]["stray"] == 0 and all(c["rK"] > 1 and c["stray"] > 0 for c in bad[1:])
    KILLS.setdefault("pod0_pos", []).append({"batch"})


def test_each_check_is_needed():
    """Runs behind the mutant tests of this module (file order).  Take one check away and a mutant survives: the ones ONLY that check saw, in every case."""
    if not all(m in KILLS for m in R.MUTANTS):
        pytest.skip("the mutant tests of this module did not all run")
    only = lambda name: sorted(m for m, seen in KILLS.items() if all(s == {name} for s in seen))   # noqa: E731
    for name in ("K", "V", "sentinel", "q", "batch"):
        print(f"seen by the {name} check alone: {', '.join(only(name))}")
    assert {"k_pos+1", "angle_next", "low_pair_neighbour", "sin_flip", "partner_swap", "head_wrap"} <= set(only("K"))
    assert only("V") == ["v_rotated"] and only("sentinel") == ["extra_row"] and only("q") == ["q_pos+1"] and only("batch") == ["pod0_pos"]


def test_zz_report():
    for (p, s, w, c), (a, b) in sorted(REPORT.items()):
        print(f"{p:9s} {s:8s} {w:4s} ctx {c:4d} float32 error/bound: textbook {a:.4f}  other order {b:.4f}")
