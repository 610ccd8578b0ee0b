"""What every QKV route of Eval leaves in the KV cache and in q, against a float64 RoPE of a float64 product, element by element
(tests/cache_probe_ref.py: the probes, the bound, the case matrix; tests/test_cache_probe_cpu.py pins the bound without a GPU).

The cache is read and written through llamago_CacheRead / llamago_CacheWrite.  Per call of a kv probe (a middle stage of TWO layers, llamago_Stage): both
slots of K and V are filled with a sentinel that depends on the offset, the call runs with the route trace on, and the whole cache is read back:
  * route: the kernel family the row count was chosen for (the trace rule of tests/test_gpu_weight_probe.py),
  * bound: rows past .. past + n - 1 of both slots inside the bound, K and V, every element,
  * sentinel: every other float of both caches bit-identical to what it held,
  * pass-through: x_out == x_in bit for bit (wo = 0, FFN 0),
  * non-finite row: the same call with its last row NaN leaves rows past .. past + n - 2 of the cache bit-identical and the last row NaN in every element,
  * reproducibility: a second context of the same model leaves the same bits.
The q probe (one layer, wo = 64 I, a host-written cache of unit keys) holds every element of x_out to its bound.  The batched part (whole two-layer models,
tok_embeddings = X) holds the rows of every pod of an lh_batch tick and feed the same way, pod by pod.

The non-finite twin found attention_gemm (prompts of 32 rows or more at a head size other than 128) spreading a NaN V row to every query of the call through
the exact zeros of its P V GEMM - first seen as kv-sparse hd64 f32 n = 64, the second layer's cache rows all NaN; fixed in csrc/kernels_gemm.h
(k_transpose_v, k_attn_gemm_repair), and test_nonfinite_v_reaches_the_queries_that_see_it holds the other half of that rule."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_probe_ref as R   # noqa: E402
from llama_go_amd.mlapi import Batch, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu

ATTN_ENTRIES = ("k_attention", "k_attn_flash", "attention_gemm", "k_softmax_causal", "k_transpose_v")
Q_CTX = 512          # the q probe needs hd + n positions (128 + 193)
REPORT = {}          # (probe, shape, wtype, family) -> [worst error / bound, calls]
TIMES = {}           # shape -> seconds spent in its tests (model builds and references included)
_MODELS = {}         # (shape, wtype, probe, ctx) -> ProbeModel: the one that is alive
_SENTINELS = {}


def rows_past(shape, wtype):
    """One row count per route family for the calls behind PAST rows: weight_probe_ref.ROWS_PAST, or the first of each family of a head-dim shape."""
    if (shape, wtype) in R.ROWS_PAST:
        return R.ROWS_PAST[shape, wtype]
    first = {}
    for n in R.HD_ROWS:
        first.setdefault(R.expected_route(shape, wtype, n)[0], n)
    return tuple(first.values())


def kv_cases():
    """(probe, shape, type, ctx, n, past) in the order they run: a probe model serves all its calls before the next one is built."""
    models = [(s, w, R.CTX, [(n, 0) for n in rows] + [(n, R.PAST) for n in R.ROWS_PAST[s, w]]) for (s, w), rows in R.ROWS.items()]
    models += [(s, w, R.CTX, [(n, 0) for n in R.HD_ROWS] + [(n, R.PAST) for n in rows_past(s, w)]) for s in R.HD_SHAPES for w in ("f32", "q8")]
    models += [("small", w, R.LONG_CTX, [(n, R.LONG_CTX - n) for n in R.LONG_ROWS]) for w in ("f32", "q8")]
    return [(p, s, w, ctx, n, past) for s, w, ctx, calls in models for p in R.KV_PROBES for n, past in calls]


def q_cases():
    """(shape, type, ctx, n, P): one row count per route family at P = hd; `small` on a context of 2048 positions, there also at P = ctx - n."""
    out = []
    for s, w in list(R.ROWS) + [(s, w) for s in R.HD_SHAPES for w in ("f32", "q8")]:
        if s == "65Blayer":                                       # (k_skinny is held by the kv probes)
            continue
        ctx = R.LONG_CTX if s == "small" else Q_CTX
        out += [(s, w, ctx, n, R.head_dim(s)) for n in rows_past(s, w)]
        if s == "small":
            out += [(s, w, ctx, n, ctx - n) for n in R.LONG_ROWS]
    return out


KV_CASES, Q_CASES = kv_cases(), q_cases()


def sentinel(which, n):
    if (which, n) not in _SENTINELS:
        _SENTINELS[which, n] = R.sentinel(which, n)
    return _SENTINELS[which, n]


class ProbeModel:
    """One probe model (a middle stage), the weights read back from it, two contexts."""

    def __init__(self, product, shape, wtype, probe, ctx):
        kw = R.SHAPES[shape]
        self.product, self.shape, self.wtype, self.probe, self.ctx = product, shape, wtype, probe, ctx
        self.d, self.H, self.S = kw["embd"], kw["heads"], (1 if probe == "q" else 2)
        hp = make_hparams(vocab=kw["vocab"], embd=kw["embd"], mult=kw["mult"], heads=kw["heads"], layers=self.S + 2, ctx=ctx)
        self.model = m = product.NewSyntheticModel(hp, 7, 1, 1 + self.S)
        assert m.ffSize == R.ff_size(kw["embd"], kw["mult"])
        names = []
        for L in range(self.S):
            T = R.probe_tensors(probe, shape, L)
            names.append({k: f"layers.{1 + L}.{v}" for k, v in R.TENSOR_NAMES.items()})
            for k, name in names[L].items():
                m.SetTensor(name, T[k])
            del T
        if wtype == "q8":
            m.QuantizeQ8()
        self.W = []
        for L in range(self.S):
            T = R.probe_tensors(probe, shape, L)
            W = {}
            for k in R.READ_BACK[probe]:
                w = product.read(None, m.tensor(names[L][k])).reshape(T[k].shape)
                if wtype == "f32" or w.ndim == 1:
                    assert np.array_equal(w, T[k]), names[L][k]
                W[k] = w
            self.W.append(W)
        self.X = R.inputs(shape, 256)
        self.ctxs = [m.NewContext(ctx, 1, False), m.NewContext(ctx, 1, False)]

    def free(self):
        for c in self.ctxs:
            c.free()
        self.model.free()


@pytest.fixture(scope="module", autouse=True)
def probe_models():
    """Frees every probe model when the module's last test is done - whatever was selected, whatever failed."""
    yield
    for k in list(_MODELS):
        _MODELS.pop(k).free()
    _SENTINELS.clear()


def get_model(product, shape, wtype, probe, ctx):
    """The cases come model by model: one probe model is alive at a time."""
    key = (shape, wtype, probe, ctx)
    if key not in _MODELS:
        for k in list(_MODELS):
            _MODELS.pop(k).free()
        _MODELS[key] = ProbeModel(product, shape, wtype, probe, ctx)
    return _MODELS[key]


def run_call(M, n, past, which=0, nan_last=False, base=None):
    """n rows at `past` on context `which` of the model, over a cache that holds the sentinel (or `base`, a pair of images)
    -> (x_out [n][d], K image, V image [S][ctx][d], trace, x_in)."""
    import torch
    c, product = M.ctxs[which], M.product
    total = M.S * M.ctx * M.d
    for kv in (0, 1):
        c.CacheWrite(kv, 0, sentinel(kv, total) if base is None else base[kv])
    x = M.X[R.call_rows(len(M.X), n, past)].copy()
    if nan_last:
        x[-1] = np.nan
    xin = torch.from_numpy(x).cuda()
    out = torch.full((n, M.d), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def stage():
        rc = product.lib.llamago_Stage(c.h, None, None, C.c_void_p(xin.data_ptr()), C.c_void_p(out.data_ptr()), n, past, None, None)
        assert rc == 0, product.last_error()

    _, trace = route_trace(stage)
    assert product.lib.llamago_Sync(c.h) == 0, product.last_error()
    K, V = (c.CacheRead(kv, 0, total).reshape(M.S, M.ctx, M.d) for kv in (0, 1))
    return out.cpu().numpy(), K, V, trace, x


def entry_name(e):
    return re.split(r"[</]", e)[0]


def check_route(trace, shape, wtype, n, layers, ctx):
    """The trace rule of tests/test_gpu_weight_probe.py for a stage of `layers` layers; on a context beyond 256 positions the decode step of a 128-wide
    head takes k_attention_split and its combine."""
    family, want, quiet = R.expected_route(shape, wtype, n)
    # a head size other than 128 takes its prompt attention through attention_gemm, whose own four launches follow its entry (csrc/plan.hip): the QK GEMM,
    # k_softmax_causal, k_transpose_v, the PV GEMM - they are attention, not weight launches
    own = set()
    for i, e in enumerate(trace):
        if e.startswith("attention_gemm/"):
            assert [entry_name(t) for t in trace[i + 1:i + 5]] == ["k_gemm_mfma", "k_softmax_causal", "k_transpose_v", "k_gemm_mfma"], (shape, wtype, n, trace[i:i + 5])
            own |= {i + 1, i + 4}
    weight = {entry_name(e) for i, e in enumerate(trace) if i not in own and e.startswith(("k_stream_", "k_gemm_", "k_gemv_cols"))}
    attn = [e for e in trace if e.startswith(ATTN_ENTRIES)]
    match = lambda name, w: name == w or (w.endswith("_") and name.startswith(w))   # noqa: E731
    if quiet:
        assert not weight, (shape, wtype, n, family, trace)
        steps = n if family == "Q8Steps" else 1                   # n single steps: the per-query attention once per row and layer
        if ctx > 256 and R.head_dim(shape) == 128 and n // steps == 1:
            assert len(attn) == 2 * steps * layers and all(e.startswith(("k_attention_split/", "k_attention_combine/")) for e in attn), (shape, wtype, n, family, attn)
        else:
            assert len(attn) == steps * layers and all(e.startswith("k_attention/") and e.endswith(f"/n{n // steps}") for e in attn), (shape, wtype, n, family, attn)
    else:
        assert all(any(match(name, w) for name in weight) for w in want) and all(any(match(name, w) for w in want) for name in weight), \
            (shape, wtype, n, family, sorted(weight))
        if want[0].startswith("k_stream_") and shape in ("small", "7Blayer", "hd64", "hd32"):
            # the passes over the weights, read from the trace: the wq|wk|wv launches in front of the first attention entry, one per pass
            first = [e for e in trace[:trace.index(attn[0])] if e.startswith(want[0])]
            assert len(first) == (2 if family.endswith("/two-pass") else 1), (shape, wtype, n, family, trace[:trace.index(attn[0]) + 1])
    return family


def report(probe, shape, wtype, family, r):
    e = REPORT.setdefault((probe, shape, wtype, family), [0.0, 0])
    e[0], e[1] = max(e[0], r), e[1] + 1


def first_bad(img, ref, key, pos):
    """(slot, row, column, error, bound) of the first element of the rows `pos` outside the bound."""
    for s in range(img.shape[0]):
        err = np.abs(img[s][pos].astype(np.float64) - ref[key][s])
        bad = np.argwhere(~(err <= ref["b" + key][s]))
        if len(bad):
            i, c = bad[0]
            return f"{len(bad)} elements of slot {s}, first (row, column) ({i}, {c}): {img[s][pos][i, c]!r} against {ref[key][s][i, c]!r}, bound {ref['b' + key][s][i, c]:.3e}"
    return ""


def check_kv_call(product, probe, shape, wtype, ctx, n, past):
    M = get_model(product, shape, wtype, probe, ctx)
    tag = f"{probe} {shape} {wtype} ctx={ctx} n={n} past={past}"
    y, K, V, trace, x = run_call(M, n, past)
    pos = past + np.arange(n)
    ref = R.kv_reference(M.W, x, pos, M.H)
    chk = R.check_cache(K, V, ref, pos)
    family = R.expected_route(shape, wtype, n)[0]
    print(f"{tag} [{family}]: K error / bound {chk['rK']:.4g}, V {chk['rV']:.4g}, stray floats {chk['stray']}; {' '.join(dict.fromkeys(entry_name(e) for e in trace))}")
    # 1. the route
    check_route(trace, shape, wtype, n, M.S, ctx)
    report(probe, shape, wtype, family, max(chk["rK"], chk["rV"]))
    # 2. the rows of the call, both slots, K and V
    assert chk["rK"] <= 1, f"{tag} [{family}]: K outside the bound (worst error / bound {chk['rK']:.3g}): {first_bad(K, ref, 'K', pos)}"
    assert chk["rV"] <= 1, f"{tag} [{family}]: V outside the bound (worst error / bound {chk['rV']:.3g}): {first_bad(V, ref, 'V', pos)}"
    # 3. every other float of both caches
    assert chk["stray"] == 0, f"{tag} [{family}]: {chk['stray']} floats outside rows {past} .. {past + n - 1} no longer hold the sentinel"
    # 4. the stage passes its input through
    assert y.tobytes() == x.tobytes(), f"{tag} [{family}]: x_out differs from x_in in {np.count_nonzero(y.view(np.uint32) != x.view(np.uint32))} elements"
    # 5. the twin with the last row NaN
    y2, K2, V2, trace2, _ = run_call(M, n, past, nan_last=True)
    assert [entry_name(e) for e in trace2] == [entry_name(e) for e in trace], tag
    assert y2[:n - 1].tobytes() == x[:n - 1].tobytes(), f"{tag} [{family}]: rows 0 .. n - 2 of x_out change when the last row is NaN (a query that does not see the NaN key took it)"
    rest = np.ones(ctx, dtype=bool)
    rest[pos] = False
    for name, a, b, kv in (("K", K, K2, 0), ("V", V, V2, 1)):
        assert b[:, pos[:-1]].tobytes() == a[:, pos[:-1]].tobytes(), f"{tag} [{family}]: rows past .. past + n - 2 of {name} change when the last row is NaN"
        assert np.all(np.isnan(b[:, pos[-1]])), f"{tag} [{family}]: {np.count_nonzero(~np.isnan(b[:, pos[-1]]))} elements of the NaN row of {name} are not NaN"
        assert b[:, rest].tobytes() == sentinel(kv, b.size).reshape(b.shape)[:, rest].tobytes(), f"{tag} [{family}]: the twin writes {name} outside its rows"
    # reproducibility: another context of the same model
    _, K3, V3, _, _ = run_call(M, n, past, which=1)
    assert K3.tobytes() == K.tobytes() and V3.tobytes() == V.tobytes(), f"{tag} [{family}]: a second context leaves other bits"


@pytest.mark.parametrize("probe,shape,wtype,ctx,n,past", KV_CASES, ids=[f"{p}-{s}-{w}-ctx{c}-n{n}-p{past}" for p, s, w, c, n, past in KV_CASES])
def test_cache_rows(product, probe, shape, wtype, ctx, n, past):
    t0 = time.time()
    try:
        check_kv_call(product, probe, shape, wtype, ctx, n, past)
    finally:
        TIMES[shape] = TIMES.get(shape, 0.0) + time.time() - t0


@pytest.mark.parametrize("shape,wtype,ctx,n,P", Q_CASES, ids=[f"q-{s}-{w}-ctx{c}-n{n}-P{P}" for s, w, c, n, P in Q_CASES])
def test_q_rows(product, shape, wtype, ctx, n, P):
    """q through the attention of a host-written cache: every element of x_out inside the bound; the call's own cache rows exactly 0, every other float
    of the cache as the host wrote it."""
    t0 = time.time()
    try:
        M = get_model(product, shape, wtype, "q", ctx)
        hd = R.head_dim(shape)
        tag = f"q {shape} {wtype} ctx={ctx} n={n} P={P}"
        base = []
        Kp, Vp = R.q_prefill(M.H, hd, P)
        for kv, rows in ((0, Kp), (1, Vp)):
            img = sentinel(kv, ctx * M.d).copy().reshape(1, ctx, M.d)
            img[0, :P] = rows
            base.append(img)
        y, K, V, trace, x = run_call(M, n, P, base=base)
        ref = R.q_reference(M.W[0], x, P, M.H)
        r = R.ratio(y, ref)
        family = R.expected_route(shape, wtype, n)[0]
        print(f"{tag} [{family}]: error / bound {r:.4g}; {' '.join(dict.fromkeys(entry_name(e) for e in trace))}")
        check_route(trace, shape, wtype, n, 1, ctx)
        report("q", shape, wtype, family, r)
        err = np.abs(y.astype(np.float64) - ref["out"])
        bad = np.argwhere(~(err <= ref["bound"]))
        assert len(bad) == 0, (f"{tag} [{family}]: {len(bad)} elements outside the bound, first (row, column) {bad[0].tolist()}: error {err[tuple(bad[0])]:.3e}, "
                               f"bound {ref['bound'][tuple(bad[0])]:.3e}; worst error / bound {r:.3g}")
        pos = P + np.arange(n)
        zero = np.zeros((1, n, M.d))
        chk = R.check_cache(K, V, dict(K=zero, V=zero, bK=zero, bV=zero), pos, base=base)
        assert chk["rK"] == 0 and chk["rV"] == 0, f"{tag} [{family}]: wk = wv = 0, but the call's own cache rows are not 0"
        assert chk["stray"] == 0, f"{tag} [{family}]: {chk['stray']} floats outside the call's rows changed"
    finally:
        TIMES[shape] = TIMES.get(shape, 0.0) + time.time() - t0


@pytest.mark.parametrize("shape", ("hd64", "hd32"))
def test_nonfinite_v_reaches_the_queries_that_see_it(product, shape):
    """The other half of the non-finite rule of attention_gemm (the twins above hold that a query which does NOT see a NaN key is untouched): a NaN the host
    writes into one V element of a key that every query of the call sees must reach every query - through wo (0 x NaN) every element of x_out is NaN.  Taking
    the value into the P V product as 0 and forgetting to add it back would leave x_out finite."""
    n, hd, H = 64, R.head_dim(shape), R.SHAPES[shape]["heads"]
    M = get_model(product, shape, "f32", "q", Q_CTX)
    base = []
    for kv, rows in enumerate(R.q_prefill(H, hd, hd)):
        img = sentinel(kv, Q_CTX * M.d).copy().reshape(1, Q_CTX, M.d)
        img[0, :hd] = rows
        base.append(img)
    y, _, _, trace, _ = run_call(M, n, hd, base=base)
    assert any(e.startswith("attention_gemm/") for e in trace) and np.all(np.isfinite(y))
    base[1][0, 3, 2 * hd + 5] = np.nan
    y2, _, _, _, _ = run_call(M, n, hd, base=base)
    assert np.all(np.isnan(y2)), f"{np.count_nonzero(~np.isnan(y2))} elements of x_out are not NaN"


def test_cache_shim_refuses_bad_arguments(product):
    """llamago_Cache*: a write reads back bit for bit at its offset; a range outside the cache, which outside 0 / 1, a pod outside the batch and a null
    pointer are errors (ml_LastError), never a copy."""
    from llama_go_amd.mlapi import MLError
    m = product.NewSyntheticModel(make_hparams(vocab=32, embd=128, mult=32, heads=2, layers=3, ctx=16), 3, 1, 3)
    try:
        c = m.NewContext(16, 1, False)
        total = 2 * 16 * 128
        try:
            assert not np.any(c.CacheRead(0, 0, total)) and not np.any(c.CacheRead(1, 0, total))      # a fresh cache is zero-filled
            v = np.arange(300, dtype=np.float32) + 0.5
            c.CacheWrite(1, total - 300, v)
            assert np.array_equal(c.CacheRead(1, total - 300, 300), v) and not np.any(c.CacheRead(1, 0, total - 300)) and not np.any(c.CacheRead(0, 0, total))
            assert c.CacheRead(0, total, 0).size == 0
            for bad in (lambda: c.CacheRead(0, total - 299, 300), lambda: c.CacheRead(0, total + 1, 0), lambda: c.CacheRead(2, 0, 4), lambda: c.CacheRead(-1, 0, 4),
                        lambda: c.CacheWrite(0, total - 3, v[:4])):
                with pytest.raises(MLError):
                    bad()
            f = product.lib.llamago_CacheRead
            vp = v.ctypes.data_as(C.POINTER(C.c_float))
            assert f(None, 0, 0, vp, 4) != 0 and f(c.h, 0, 0, None, 4) != 0 and "null" in product.last_error()
            assert f(c.h, 0, 2 ** 63, vp, 2 ** 63) != 0 and f(c.h, 0, 8, vp, 2 ** 64 - 4) != 0 and "outside" in product.last_error()      # (off + n wraps)
            assert np.array_equal(c.CacheRead(1, total - 300, 300), v)
        finally:
            c.free()
    finally:
        m.free()
    m = product.NewSyntheticModel(make_hparams(vocab=32, embd=128, mult=32, heads=2, layers=2, ctx=16), 3)
    try:
        b = Batch(m, 16, 2)
        try:
            v = np.arange(128, dtype=np.float32) - 7
            b.CacheWrite(1, 0, 128, v)
            assert np.array_equal(b.CacheRead(1, 0, 128, 128), v) and not np.any(b.CacheRead(0, 0, 0, total)) and not np.any(b.CacheRead(1, 1, 0, total))
            for bad in (lambda: b.CacheRead(2, 0, 0, 4), lambda: b.CacheWrite(2, 0, 0, v), lambda: b.CacheRead(0, 0, total - 1, 2), lambda: b.CacheRead(0, 3, 0, 4)):
                with pytest.raises(MLError):
                    bad()
        finally:
            b.free()
    finally:
        m.free()


# ---- batched Eval ------------------------------------------------------------------------------------------------------------------------------
BATCH_MODELS = (("small", "f32"), ("small", "q8"), ("hd32", "f32"))
BATCH_PODS = (3, 16, 64)
FEED_LENGTHS = (1, 5, 40, 0, 2, 9, 1, 3)


def batch_plans(pods):
    """[(kind, tokens per pod, past per pod)]: ticks at pairwise different positions that hold 0, 1, 7 and 255, feeds of mixed lengths (0, 1, 5 and 40
    among them) at different positions.  Token id = row of X; no id twice in a call."""
    if pods == 3:
        ticks = [[0, 1, 255], [7, 255, 0]]
    else:
        ticks = [[0, 1, 7, 255] + [11 + 3 * i for i in range(pods - 4)]]
    plans = [("tick", [[5 + 31 * k + i] for i in range(pods)], p) for k, p in enumerate(ticks)]
    for shift in (0, 3):
        lens = [FEED_LENGTHS[(i + shift) % len(FEED_LENGTHS)] for i in range(pods)]
        past = [(0, 1, 7)[i % 3] + 5 * (i // 3) for i in range(pods)]
        last = max(i for i in range(pods) if lens[i])
        past[last] = R.CTX - lens[last]                           # one pod up to the window's last position
        start = np.cumsum([0] + lens)
        plans.append(("feed", [list(range(100 + start[i], 100 + start[i] + lens[i])) for i in range(pods)], past))
    return plans


@pytest.fixture(scope="module", params=BATCH_MODELS, ids=[f"{s}-{w}" for s, w in BATCH_MODELS])
def batch_model(request, product):
    """A whole two-layer model of kv-sparse layers whose embedding table is X: token id = row index."""
    shape, wtype = request.param
    for k in list(_MODELS):                                       # (the stage models of the tests above are done)
        _MODELS.pop(k).free()
    kw = R.SHAPES[shape]
    hp = make_hparams(vocab=kw["vocab"], embd=kw["embd"], mult=kw["mult"], heads=kw["heads"], layers=2, ctx=R.CTX)
    m = product.NewSyntheticModel(hp, 7)
    try:
        m.SetTensor("tok_embeddings.weight", R.inputs(shape, kw["vocab"]))
        names = []
        for L in range(2):
            T = R.probe_tensors("kv-sparse", shape, L)
            names.append({k: f"layers.{L}.{v}" for k, v in R.TENSOR_NAMES.items()})
            for k, name in names[L].items():
                m.SetTensor(name, T[k])
        if wtype == "q8":
            m.QuantizeQ8()
        W = [{k: product.read(None, m.tensor(names[L][k])).reshape((kw["embd"], -1) if k != "g1" else (-1,)) for k in R.READ_BACK["kv-sparse"]} for L in range(2)]
        X = product.read(None, m.tensor("tok_embeddings.weight")).reshape(kw["vocab"], kw["embd"])
        assert np.all(np.isfinite(X)) and len(np.unique(X[:, 0])) > kw["vocab"] // 2
        yield shape, wtype, m, W, X
    finally:
        m.free()


@pytest.mark.parametrize("pods", BATCH_PODS)
def test_batched_eval_cache_rows(product, batch_model, pods):
    """lh_batch ticks and feeds: pod i's rows at pod i's positions of pod i's cache inside the bound, every other float of every pod's cache the sentinel."""
    shape, wtype, m, W, X = batch_model
    kw = R.SHAPES[shape]
    d, H, total = kw["embd"], kw["heads"], 2 * R.CTX * kw["embd"]
    t0 = time.time()
    b = Batch(m, R.CTX, pods)
    try:
        for kind, tokens, past in batch_plans(pods):
            assert all(p + len(t) <= R.CTX for t, p in zip(tokens, past)) and len({i for t in tokens for i in t}) == sum(len(t) for t in tokens)
            if kind == "tick":
                assert len(set(past)) == pods
            for i in range(pods):
                for kv in (0, 1):
                    b.CacheWrite(i, kv, 0, sentinel(kv, total))
            if kind == "tick":
                b.Set([t[0] for t in tokens], past)
                _, trace = route_trace(b.Tick)
            else:
                _, trace = route_trace(lambda: b.Feed(tokens, past))
            worst, names = 0.0, " ".join(dict.fromkeys(entry_name(e) for e in trace))
            for i in range(pods):
                K, V = (b.CacheRead(i, kv, 0, total).reshape(2, R.CTX, d) for kv in (0, 1))
                pos = past[i] + np.arange(len(tokens[i]))
                ref = R.kv_reference(W, X[tokens[i]], pos, H) if len(pos) else dict(K=np.zeros((2, 0, d)), V=np.zeros((2, 0, d)), bK=np.zeros((2, 0, d)), bV=np.zeros((2, 0, d)))
                chk = R.check_cache(K, V, ref, pos)
                tag = f"batch {kind} {shape} {wtype} pods={pods} pod {i} ({len(pos)} rows at {past[i]})"
                assert chk["rK"] <= 1, f"{tag}: K outside the bound (worst error / bound {chk['rK']:.3g}): {first_bad(K, ref, 'K', pos)}; {names}"
                assert chk["rV"] <= 1, f"{tag}: V outside the bound (worst error / bound {chk['rV']:.3g}): {first_bad(V, ref, 'V', pos)}; {names}"
                assert chk["stray"] == 0, f"{tag}: {chk['stray']} floats outside the pod's rows no longer hold the sentinel; {names}"
                worst = max(worst, chk["rK"], chk["rV"])
            print(f"batch {kind} {shape} {wtype} pods={pods} rows={sum(len(t) for t in tokens)}: worst error / bound {worst:.4g}; {names}")
            report("kv-sparse", shape, wtype, f"batch-{kind}/pods{pods}", worst)
    finally:
        b.free()
        TIMES[shape] = TIMES.get(shape, 0.0) + time.time() - t0


def test_zz_report():
    """Prints (and, with CACHE_PROBE_REPORT set, writes) the worst error / bound per (probe, shape, type, route family) of this session and the seconds
    each shape's tests took: the source of profiles/cache_probe.txt."""
    lines = [f"{p:9s} {s:10s} {w:4s} {fam:26s} calls {n:3d}   worst error/bound {br:.4f}" for (p, s, w, fam), (br, n) in sorted(REPORT.items())]
    lines += [f"seconds in the tests of {s}: {t:.1f}" for s, t in sorted(TIMES.items())]
    print("\n".join(lines))
    path = os.environ.get("CACHE_PROBE_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
