"""Q4_1 models (dtype 3): the quantiser and the value of a weight bit for bit, every native launch against float64, the expanded routes against the fp32
model of the same values by bytes, rows against steps, and the file round trip.  The value of a weight is w' = fl32(fma(d, n, m)) (tests/q41_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q41_ref as Q   # noqa: E402
import weight_probe_ref as R   # noqa: E402
from test_gpu_weight_probe import run_call   # noqa: E402  (n rows through a stage of a probe model, with the route trace)
from test_gpu_q4 import FILE_SMALL_PROMPT, parse_ggjt, refusal, write_ggjt   # noqa: E402  (ggjt files as (head, tensors); the message of a refused load)
from llama_go_amd.mlapi import SHAPES, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu

Q41_KERNELS = ("k_gemv_q41s", "k_gemv_q41_rows", "k_expand_q41", "k_quantize_q41", "k_q41_deinterleave")
SMALL = R.SHAPES["small"]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def families(trace):
    return [e.split("<")[0].split("/")[0] for e in trace]


def cache_rows(c, hp, pos, n):
    """rows pos .. pos + n - 1 of K and V, both layers"""
    return [c.CacheRead(which, (layer * 256 + pos) * hp.embdSize, n * hp.embdSize).tobytes() for which in (0, 1) for layer in (0, 1)]


def same_values(got, want):
    """bit-equal floats, any NaN for a NaN"""
    got, want = np.ravel(got).astype(np.float32), np.ravel(want).astype(np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and same(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


# ---- 1. quantiser and values ---------------------------------------------------------------------------------------------------------------------------
def test_quantiser_blocks_and_values_bit_for_bit(product):
    hp = make_hparams(vocab=64, embd=256, mult=32, heads=2, layers=1, ctx=16)
    m = product.NewSyntheticModel(hp, 3)
    try:
        rng = np.random.default_rng(4)
        w = (rng.standard_normal((256, 256)) * 2.0 ** rng.integers(-6, 3, (256, 1))).astype(np.float32)
        w[:9, :32] = Q.crafted_blocks()
        name = "layers.0.attention.wq.weight"
        m.SetTensor(name, w)
        _, tr = route_trace(m.QuantizeQ41)
        assert m.weight_type == 3 and "k_quantize_q41" in tr
        d, mn, n = Q.quantize(w)
        got = m.blocks_q41(name, w.size)
        want = Q.to_blocks(d, mn, n)
        gd, gm, gn = Q.from_blocks(got, 256, 256)
        assert same(gn, n) and same_values(gd, d) and same_values(gm, mn)
        finite = np.isfinite(d).ravel()
        assert same(got[finite], want[finite])
        values = product.read(None, m.tensor(name))
        assert same_values(values, Q.dequantize(d, mn, n))
        _, tr = route_trace(m.ExpandQ41)
        assert m.weight_type == 0 and "k_expand_q41" in tr
        assert same_values(product.read(None, m.tensor(name)), values)       # the expanded model holds the bytes of that read
    finally:
        m.free()


# ---- 2. every native launch against float64 --------------------------------------------------------------------------------------------------------------
class Q41Probe:
    """tests/test_gpu_weight_probe.py's Probe with the matrices quantised to Q4_1: W is the fp32 read-back, the weights' values themselves"""

    def __init__(self, product, shape, probe):
        kw = R.SHAPES[shape]
        self.shape, self.probe, self.d, self.V = shape, probe, kw["embd"], kw["vocab"]
        layer = 2 if probe == "head" else 1
        self.model = m = product.NewSyntheticModel(make_hparams(vocab=kw["vocab"], embd=kw["embd"], mult=kw["mult"], heads=kw["heads"], layers=3, ctx=R.CTX), 7, layer, layer + 1)
        T = R.probe_tensors(probe, shape)
        names = {k: f"layers.{layer}.{v}" for k, v in R.TENSOR_NAMES.items()}
        if probe == "head":
            names.update(norm="norm.weight", output="output.weight")
        for k, name in names.items():
            m.SetTensor(name, T[k])
        m.QuantizeQ41()
        W = {k: product.read(None, m.tensor(name)).reshape(T[k].shape) for k, name in names.items()}
        for k in R.ZERO[probe]:
            assert not np.any(W[k]), (probe, shape, k)
        self.X = R.inputs(shape, R.PAST + 4)
        self.ref = R.reference(probe, W, self.X)


NATIVE = [(s, p) for s in ("small", "7Blayer", "65Blayer") for p in R.probes_of(s)]


@pytest.mark.parametrize("shape,probe", NATIVE, ids=[f"{p}-{s}" for s, p in NATIVE])
def test_native_launches_against_float64(product, shape, probe):
    """ratio <= 1 under the a-priori bound C u |W||z| of tests/weight_probe_ref.py - W holds the values w', so reference and bound apply unchanged - on
    k_gemv_q41s (n = 1) and k_gemv_q41_rows (n = 2..4), and no expansion in front of them.  small: the 256-thread KI = 1 forms; 7Blayer: KI = 1 and 3, 256 threads;
    65Blayer (K / 16 = 512 and 1376, no row kernel of that width: one row only): the 1024-thread forms k_gemv_q41s<2,2,256> and <2,2,1024>."""
    P = Q41Probe(product, shape, probe)
    try:
        for n, past in [(1, 0)] if shape == "65Blayer" else [(1, 0), (2, 0), (3, 0), (4, 0), (1, R.PAST), (4, R.PAST)]:
            y, trace = run_call(product, P, n, past)
            rows = slice(past + n - 1, past + n) if probe == "head" else slice(past, past + n)
            ratio = R.ratio(y, dict(out=P.ref["out"][rows], bound=P.ref["bound"][rows]))
            names = set(families(trace))
            print(f"{probe} {shape} n={n} past={past}: error / bound {ratio:.4g}; {sorted(names)}")
            assert ratio <= 1.0, (probe, shape, n, past, ratio)
            assert "k_expand_q41" not in names and not any(e.startswith(("k_stream_", "k_gemm_", "k_gemv_cols")) for e in names), trace
            assert shape != "65Blayer" or any(e.startswith("k_gemv_q41s<") and e.endswith(",1024>") for e in trace), trace
            if probe == "head" or n == 1:      # (the head's one logits row is a k_gemv_q41s launch behind any row count)
                assert "k_gemv_q41s" in names, trace
            if n > 1 and probe != "head":
                assert "k_gemv_q41_rows" in names and "k_gemv_q41s" not in names, trace
    finally:
        P.model.free()


# ---- 3 - 5: whole models ---------------------------------------------------------------------------------------------------------------------------------
def twins(product, hp, seed=77):
    """(A, B): the same synthetic values as Q4_1 and as the fp32 model of those very blocks' values"""
    A, B = product.NewSyntheticModel(hp, seed).QuantizeQ41(), product.NewSyntheticModel(hp, seed).QuantizeQ41().ExpandQ41()
    assert (A.weight_type, B.weight_type) == (3, 0)
    return A, B


@pytest.fixture(scope="module")
def small_twins(product):
    hp = make_hparams(**SMALL, layers=2, ctx=256)
    A, B = twins(product, hp)
    yield hp, A, B
    A.free(); B.free()


@pytest.mark.parametrize("n", [5, 9, 49, 65, 129, 193])
def test_expanded_route_is_the_fp32_route(small_twins, n):
    """the last-row logits of the contract route and every cache row A wrote are B's bytes; A's launches are B's behind k_expand_q41 passes"""
    hp, A, B = small_twins
    ca, cb = A.NewContext(256, 1), B.NewContext(256, 1)
    try:
        toks = [int(t) for t in np.random.default_rng(n).integers(0, hp.vocabSize, n)]
        la, ta = route_trace(lambda: ca.Eval(toks, 3))
        lb, tb = route_trace(lambda: cb.Eval(toks, 3))
        assert np.isfinite(lb).all() and np.abs(lb).max() > 0
        assert same(la, lb), (n, float(np.abs(la - lb).max()))
        assert cache_rows(ca, hp, 3, n) == cache_rows(cb, hp, 3, n), n
        fa = families(ta)
        assert fa.count("k_expand_q41") >= 14 and not set(fa) & {"k_gemv_q41s", "k_gemv_q41_rows"}, ta
        assert not set(families(tb)) & set(Q41_KERNELS), tb
        assert [e for e in ta if e.split("<")[0] not in Q41_KERNELS] == tb, n
    finally:
        ca.free(); cb.free()


@pytest.mark.parametrize("n", [2, 3, 4])
def test_rows_of_a_verify_pass_equal_single_steps(small_twins, n):
    """row i of an n-row pass = the one-token Eval at its position, by bytes: a pass whose draft is wrong behind row i stops there and returns that row's
    logits; the pass that accepts every draft leaves every row's K and V"""
    hp, A, _ = small_twins
    cv, cs = A.NewContext(256, 1), A.NewContext(256, 1)
    try:
        prompt = [int(t) for t in np.random.default_rng(20 + n).integers(0, hp.vocabSize, 6)]
        P = len(prompt)
        first = int(np.argmax(cv.Eval(prompt, 0)))
        assert int(np.argmax(cs.Eval(prompt, 0))) == first
        steps, ids, tok = [], [], first                          # n greedy one-token steps: their ids are the drafts every row accepts
        for i in range(n):
            steps.append(cs.Eval([tok], P + i))
            tok = int(np.argmax(steps[-1]))
            ids.append(tok)
        for i in range(n):                                       # (the last pass, i = n - 1, accepts every draft)
            toks = [first] + ids[:n - 1]
            if i < n - 1:
                toks[i + 1] = (ids[i] + 1) % hp.vocabSize
            (got, a, lg), tr = route_trace(lambda: cv.Verify(toks, P, want_logits=True))
            assert "k_gemv_q41_rows" in families(tr) and "k_expand_q41" not in families(tr), tr
            assert a == i and list(got) == ids[:i + 1]
            assert same(lg, steps[i]), (n, i)
        assert cache_rows(cv, hp, P, n) == cache_rows(cs, hp, P, n), n
    finally:
        cv.free(); cs.free()


# ---- 5. files ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_files(product, tmp_path_factory):
    """tiny twins, A saved as Q4_1 and B as f32, and the Q4_1 file as write_ggjt's (head, tensors): B's file parsed (parse_ggjt knows no dtype 3), its
    matrices replaced by A's blocks - written back it must be A's file byte for byte"""
    hp = make_hparams(**SHAPES["tiny"], ctx=32)
    A, B = twins(product, hp, seed=21)
    d = tmp_path_factory.mktemp("q41")
    path, plain = str(d / "q41.bin"), str(d / "f32.bin")
    A.SaveQ41(path)
    B.Save(plain, 0)
    _, tensors, head = parse_ggjt(plain)
    head = open(path, "rb").read()[:len(head)]
    for name, (_, ne, _) in list(tensors.items()):
        if len(ne) == 2 and name != "tok_embeddings.weight":
            tensors[name] = (3, ne, A.blocks_q41(name, ne[0] * ne[1]).tobytes())
    write_ggjt(str(d / "again.bin"), head, tensors)
    assert open(str(d / "again.bin"), "rb").read() == open(path, "rb").read()
    yield hp, A, B, path, plain, tensors, head, d
    A.free(); B.free()


@pytest.mark.parametrize("case", ["whole", "f32_file", "one_f16_matrix", "output_f16", "one_matrix_missing"])
def test_files(product, tiny_files, case):
    """whole: llama_LoadModel refuses the Q4_1 file as the reference does.  f32_file: a file without Q4_1 matrices loads as ever.  The other cases: a Q4_1
    file in which ONE of the 7 L + 1 matrices is f16 (in the middle of the file, or the output matrix) or is not there - LoadModelKeepQ41's look over
    the headers hands it to llama_LoadModel's own load, whose refusal it is.  Behind each: the whole file loads, block for block, and evaluates as A."""
    hp, A, B, path, plain, tensors, head, d = tiny_files
    if case == "whole":
        assert "not supported" in refusal(lambda: product.LoadModel(path, 32))
    elif case == "f32_file":
        W = product.LoadModelKeepQ41(plain, 32)
        cw, cb = W.NewContext(32, 1), B.NewContext(32, 1)
        try:
            assert W.weight_type == 0 and same(cw.Eval(FILE_SMALL_PROMPT, 0), cb.Eval(FILE_SMALL_PROMPT, 0))
        finally:
            cw.free(); cb.free(); W.free()
    else:
        mixed_t = dict(tensors)
        victim = "output.weight" if case == "output_f16" else "layers.1.feed_forward.w1.weight"
        assert mixed_t[victim][0] == 3
        if case == "one_matrix_missing":
            del mixed_t[victim]
        else:
            mixed_t[victim] = (1, mixed_t[victim][1], product.read(None, B.tensor(victim)).astype(np.float16).tobytes())
        mixed = str(d / f"{case}.bin")
        write_ggjt(mixed, head, mixed_t)
        want, kept = refusal(lambda: product.LoadModel(mixed, 32)), refusal(lambda: product.LoadModelKeepQ41(mixed, 32))
        assert kept.replace("llamago_LoadModelKeepQ41", "llama_LoadModel") == want and "not supported" in want, (kept, want)
    K, tr = route_trace(lambda: product.LoadModelKeepQ41(path, 32))      # (nothing half-registered stands in the way)
    ca, ck = A.NewContext(32, 1), K.NewContext(32, 1)
    try:
        assert K.weight_type == 3 and "k_q41_deinterleave" in tr
        assert all(dt == 0 or K.blocks_q41(name, ne[0] * ne[1]).tobytes() == raw for name, (dt, ne, raw) in tensors.items())
        assert same(ck.Eval(FILE_SMALL_PROMPT, 0), ca.Eval(FILE_SMALL_PROMPT, 0))
    finally:
        ca.free(); ck.free(); K.free()
