"""not-gpu: what tests/test_gpu_sample_lookup.py rests on, checked without a device.
 - the ring view of a row (tests/sample_lookup_cases.py, written from the header's rule) equals literal sequential appends;
 - the checker's own sampled runs of the loop cases contain what the GPU tests assert: accepted drafts with the replay corpus, a pass accepted
   in part with the corrupted one, other ids with the second seed, a penalty that matters;
 - the new entry points are declared and exported, and nothing of them works without a context or a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_lookup_cases as sc
import speculative_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_NAMES = ("lh_sample_rows", "lh_llama_decode_sample_lookup")
GO_NAMES = ("llamago_SampleRows", "llamago_SampleDecodeLookup")


# ---- the ring view ----------------------------------------------------------------------------------------------------------------------------
def test_ring_view_equals_literal_appends_on_random_cases():
    rng = np.random.default_rng(5)
    seen_small = 0
    for _ in range(4000):
        rs = int(rng.choice([1, 2, 3, 5, 8, 128]))
        pos = int(rng.choice([0, rs - 1, rs, 3 * rs + 2, int(rng.integers(0, 4 * rs + 1))]))
        ring, pos = sc.ring_after(rng.integers(0, 50, pos), rs)
        rows = int(rng.integers(1, 9))
        tokens = [int(t) for t in rng.integers(0, 50, rows)]
        for r in range(rows):
            assert sorted(sc.ring_view(ring, pos, tokens, r)) == sorted(sc.ring_view_literal(ring, pos, tokens, r)), (rs, pos, tokens, r)
            seen_small += rs < r
    assert seen_small > 100          # slots overwritten more than once were among the cases


def test_ring_view_hand_cases():
    assert sc.ring_view([7], 4, [9, 1, 2, 3], 3) == [3]                                   # one slot: only the last append is left
    assert sorted(sc.ring_view([5, 6], 1, [9, 1, 2, 3], 3)) == [2, 3]                     # slot 1 written twice (1 then 3), slot 0 once
    assert sorted(sc.ring_view([5, 0, 0], 1, [9, 4], 1)) == [0, 4, 5]                     # ring_pos < ring_size: an initial zero stays a member
    assert sorted(sc.ring_view([5, 6, 7], 3, [9, 4], 0)) == [5, 6, 7]                     # row 0: the ring as it is
    assert sc.ring_after([1, 2, 3, 4, 5], 3) == ([4, 5, 3], 5)


# ---- the checker's runs of the loop cases -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(built):
    from llama_go_amd.mlapi import MLLib
    return MLLib(os.path.join(ROOT, "oracle", "liboracle.so"))


def _run(lib, ctx, int8, prompt, n, seed, keep=0, **kw):
    from llama_go_amd.mlapi import make_hparams
    m = lib.NewSyntheticModel(make_hparams(**sc.HD128, ctx=ctx), sc.MODEL_SEED)
    if int8:
        m.QuantizeQ8()
    c = m.NewContext(ctx, 4)
    c.SetKeepCount(keep)
    out = c.SampleDecode(prompt, n, seed=seed, **dict(sc.SMP, **kw))
    c.free()
    m.free()
    return out


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
@pytest.mark.parametrize("ctx", [256, 384])
def test_checker_runs_hold_what_the_gpu_tests_assert(checker, ctx, int8):
    V, K, n = sc.HD128["vocab"], sc.kmax(int8), sc.N_PREDICT
    prompt = sc.prompt_for(V, 8)
    runs = [_run(checker, ctx, int8, prompt, n, seed) for seed in sc.LOOP_SEEDS]
    assert runs[0] != runs[1], "the second seed must give other ids"
    for run in runs:
        tr, st = ref.simulate(prompt + [run[0]], run[1:], n - 1, K, 3, 1, prompt + run, ctx, V)
        assert st["accepted"] > 0 and st["passes"] < n - 1, st
        tr, st = ref.simulate(prompt + [run[0]], run[1:], n - 1, K, 2, 1, sc.corrupted(prompt + run, len(prompt), V), ctx, V)
        assert any(a < k for k, a in tr), tr                                               # a pass of 0 <= a < k


def test_checker_penalty_matters(checker):
    prompt = sc.prompt_for(sc.HD128["vocab"], 8)
    a = _run(checker, 256, False, prompt, sc.N_PREDICT, 99, topK=1, repeatPenalty=1.5)
    b = _run(checker, 256, False, prompt, sc.N_PREDICT, 99, topK=1, repeatPenalty=1.0)
    assert a != b


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_checker_runs_at_the_window_end_accept_drafts(checker, int8):
    V, K = sc.HD128["vocab"], sc.kmax(int8)
    prompt = sc.prompt_for(V, 256 - 13, seed=11)
    run = _run(checker, 256, int8, prompt, 40, 99, keep=8)
    _, st = ref.simulate(prompt + [run[0]], run[1:], 39, K, 3, 1, prompt + run, 256, V, 8)
    assert st["accepted"] > 0
    prompt = sc.prompt_for(V, 8)
    run = _run(checker, 64, int8, prompt, 101, 99, keep=8)
    _, st = ref.simulate(prompt + [run[0]], run[1:], 100, K, 3, 1, prompt + run, 64, V, 8)
    assert st["accepted"] > 0 and st["passes"] < 100


# ---- exports, headers, loud failure -----------------------------------------------------------------------------------------------------------
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_entry_points_are_declared_and_exported(built):
    import llama_go_amd as pkg
    hip_hdr, ext_hdr = _header("llamahip.h"), _header("llamago_ext.h")
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    for n in HIP_NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hip_hdr), f"include/llamahip.h does not declare {n}"
        assert hasattr(hip, n), f"libllamahip.so does not export {n}"
    go = C.CDLL(pkg.LIBLLAMAGO)
    product_part = open(os.path.join(ROOT, "include", "llamago_ext.h")).read().split("[product] device plumbing", 1)[1]
    for n in GO_NAMES:
        assert re.search(r"\b" + n + r"\s*\(", ext_hdr) and re.search(r"\b" + n + r"\s*\(", product_part), f"include/llamago_ext.h does not declare {n} in its [product] part"
        assert hasattr(go, n), f"libllamago.so does not export {n}"
    shim = open(os.path.join(ROOT, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    assert re.search(r"\bC\.lh_llama_decode_sample_lookup\s*\(", shim) and "DecodeSampleLookup" in shim
    # the header states the rule
    raw = open(os.path.join(ROOT, "include", "llamahip.h")).read()
    for phrase in ("ring view of row r", "draw of row r", "commit:"):
        assert phrase in raw, phrase


def test_fails_loudly_without_a_context_or_a_gpu(built):
    import llama_go_amd as pkg
    from llama_go_amd.mlapi import LookupParams, MLError, SpecStats, load_product, sample_rows
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    hip.lh_sample_rows.restype = hip.lh_llama_decode_sample_lookup.restype = C.c_int
    hip.lh_sample_rows.argtypes = [C.c_void_p, f32p, C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u32p, C.c_void_p, C.c_uint64, u32p]
    hip.lh_llama_decode_sample_lookup.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(LookupParams), u32p,
                                                  C.POINTER(SpecStats), C.POINTER(C.c_uint16), C.c_uint32]
    lg, one, out = (C.c_float * 8)(), (C.c_uint32 * 1)(0), (C.c_uint32 * 8)()
    assert hip.lh_sample_rows(None, lg, 1, 8, one, 1, 0, one, None, 0, out) == -1           # LH_EINVAL
    assert hip.lh_llama_decode_sample_lookup(None, one, 1, 1, 1, None, None, out, None, None, 0) == -1
    prod = load_product()
    prod.lib.llamago_SampleDecodeLookup.restype = C.c_int
    prod.lib.llamago_SampleDecodeLookup.argtypes = [C.c_void_p, C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                                    C.c_uint64, C.POINTER(LookupParams), u32p, C.POINTER(SpecStats), C.POINTER(C.c_uint16), C.c_uint32]
    assert prod.lib.llamago_SampleDecodeLookup(None, None, one, 1, 1, 0, 40, 0.95, 0.8, 1.1, 0, None, out, None, None, 0) != 0
    assert b"llamago_SampleDecodeLookup" in prod.lib.ml_LastError()
    hip.lh_device_count.restype = C.c_int
    if hip.lh_device_count() == 0:
        with pytest.raises(MLError, match="no HIP"):
            sample_rows(prod, np.zeros((1, 8), np.float32), [0], 0, [0])
