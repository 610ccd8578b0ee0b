"""Every fused weight launch of Eval against a float64 product, element by element (tests/weight_probe_ref.py: the probes, the bound, the case matrix).

A probe layer (llamago_SetModelTensor, then QuantizeQ8 for block-int8) lets ONE matrix of the layer be dense and random and makes every other one 0, an
identity, a fold or a spread, so that a middle pipeline stage (llamago_Stage -> plan_eval) shows that matrix' product in every element of every row of
x_out - with the RMSNorm gain prologue, the row map (wq|wk|wv, w1|w3), the epilogue (cache append, silu mul, residual) and the K-split reduce of the launch
that carries it.  The `head` probe does the same for the lm_head through the logits of a last stage.  The reference takes the weights as read back from the
device (block-int8: fl32(d q)).  Per call (n rows at past = 0 on a fresh context, and once per route behind seven cached rows):
  * route: the trace shows the kernel family the row count was chosen for (Step, Rows, Q8Steps and k_skinny name no GEMV launch: then no k_stream_ /
    k_gemm_ entry may appear and the attention is the per-query one),
  * bound: every element of every row inside the bound,
  * non-finite row: the same call with its last row all NaN leaves rows 0 .. n - 2 bit-identical and row n - 1 NaN in every element.
The quantiser k_quantize_q8 is held bit for bit to the numpy restatement of its rule on crafted blocks, non-finite ones included."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_probe_ref as R   # noqa: E402
from llama_go_amd.mlapi import make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu

BIG = ("7Blayer", "65Blayer")
ATTN_ENTRIES = ("k_attention", "k_attn_flash", "attention_gemm", "k_softmax_causal", "k_transpose_v")
REPORT = {}      # (probe, shape, wtype, family) -> [worst error / bound, calls]
TIMES = {}       # shape -> seconds spent in its tests (model builds and references included)
_PROBES = {}     # (shape, wtype, probe) -> Probe; the small ones stay for the session, one big one at a time


def case_list():
    """(shape, type, probe, n, past, check) in the order they run: a probe model serves all its calls, the bound checks and then their non-finite twins,
    before the next one is built (the 7B and 65B layers are built once per probe and freed)."""
    out = []
    for (shape, wtype), rows in R.ROWS.items():
        for probe in R.probes_of(shape):
            calls = [(n, 0) for n in rows] + [(n, R.PAST) for n in R.ROWS_PAST[shape, wtype]]
            out += [(shape, wtype, probe, n, past, "bound") for n, past in calls]
            if probe != "head":                                   # (the head shows only the last row)
                out += [(shape, wtype, probe, n, past, "nan") for n, past in calls]
    return out


CASES = case_list()


class Probe:
    """One probe model, the weights read back from it, and the reference of every row of the shape's X."""

    def __init__(self, product, shape, wtype, probe):
        kw = R.SHAPES[shape]
        self.shape, self.wtype, self.probe, self.d, self.V = shape, wtype, probe, kw["embd"], kw["vocab"]
        hp = make_hparams(vocab=kw["vocab"], embd=kw["embd"], mult=kw["mult"], heads=kw["heads"], layers=3, ctx=R.CTX)
        layer = 2 if probe == "head" else 1                       # head: the last stage; else a middle one
        self.model = m = product.NewSyntheticModel(hp, 7, layer, layer + 1)
        assert m.ffSize == R.ff_size(kw["embd"], kw["mult"])
        T = R.probe_tensors(probe, shape)
        names = {k: f"layers.{layer}.{v}" for k, v in R.TENSOR_NAMES.items()}
        if probe == "head":
            names.update(norm="norm.weight", output="output.weight")
        for k, name in names.items():
            m.SetTensor(name, T[k])
        if wtype == "q8":
            m.QuantizeQ8()
        W = {}
        for k, name in names.items():
            w = product.read(None, m.tensor(name)).reshape(T[k].shape)
            if k in R.ZERO[probe]:
                assert not np.any(w), f"{probe} {shape} {wtype}: {name} must read back as exactly 0"
                w = np.zeros(T[k].shape, dtype=np.float32)        # (untouched pages: the read-back copy is dropped)
            elif wtype == "f32" or w.ndim == 1:
                assert np.array_equal(w, T[k]), name
            W[k] = w
        self.X = R.inputs(shape, R.total_rows(shape, wtype))
        self.ref = R.reference(probe, W, self.X)                  # the weights are not kept: the reference of every row is

    def free(self):
        self.model.free()


@pytest.fixture(scope="module", autouse=True)
def probe_models():
    """Frees every probe model and drops the kept outputs when the module's last test is done - whatever was selected, whatever failed."""
    yield
    for k in list(_PROBES):
        _PROBES.pop(k).free()
    _CLEAN.clear()


def get_probe(product, shape, wtype, probe):
    key = (shape, wtype, probe)
    if key not in _PROBES:
        for k in [k for k in _PROBES if k[0] in BIG]:             # one big model at a time
            _PROBES.pop(k).free()
        for k in [k for k in _CLEAN if k[:3] != key]:             # (the twins of a probe's calls run right behind them: only its own outputs are kept)
            del _CLEAN[k]
        _PROBES[key] = Probe(product, shape, wtype, probe)
    return _PROBES[key]


SENTINEL = 12345.0   # what the output buffer of a non-finite twin holds before the call: a NaN row there is a row the kernel wrote


def run_call(product, P, n, past, nan_last=False):
    """n rows at `past` on a fresh context (behind `past` unchecked rows) -> (x_out [n][d], or the logits [1][V] of the last row for `head`; trace).
    The output buffer is pre-filled with NaN (an element the call leaves unwritten fails the bound), with SENTINEL when the last row is NaN."""
    import torch
    head = P.probe == "head"
    c = P.model.NewContext(R.CTX, 1, False)
    try:
        x = P.X[:past + n].copy()
        if nan_last:
            x[-1] = np.nan
        xin = torch.from_numpy(x).cuda()
        out = torch.full((1, P.V) if head else (n, P.d), SENTINEL if nan_last else float("nan"), dtype=torch.float32, device="cuda")
        scratch = torch.empty((max(past, 1), P.d), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def stage(src, n_rows, at, dst, logits):
            rc = product.lib.llamago_Stage(c.h, None, None, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()) if dst is not None else None, n_rows, at,
                                           C.c_void_p(logits.data_ptr()) if logits is not None else None, None)
            assert rc == 0, product.last_error()

        if past:
            stage(xin, past, 0, None if head else scratch, None)
        _, trace = route_trace(lambda: stage(xin[past], n, past, None if head else out, out if head else None))
        assert product.lib.llamago_Sync(c.h) == 0, product.last_error()
        return out.cpu().numpy(), trace
    finally:
        c.free()


def entry_name(e):
    return re.split(r"[</]", e)[0]


def check_route(trace, shape, wtype, n, last):
    family, want, quiet = R.expected_route(shape, wtype, n, last)
    weight = {entry_name(e) for e in trace if e.startswith(("k_stream_", "k_gemm_", "k_gemv_cols"))}
    attn = [e for e in trace if e.startswith(ATTN_ENTRIES)]
    match = lambda name, w: name == w or (w.endswith("_") and name.startswith(w))   # noqa: E731
    if quiet:
        assert not weight, (shape, wtype, n, family, trace)
        steps = n if family == "Q8Steps" else 1                   # n single steps: the per-query attention once per row
        assert len(attn) == steps and all(e.startswith("k_attention/") and e.endswith(f"/n{n // steps}") for e in attn), (shape, wtype, n, family, attn)
    else:
        assert all(any(match(name, w) for name in weight) for w in want) and all(any(match(name, w) for w in want) for name in weight), \
            (shape, wtype, n, family, sorted(weight))
        if want[0].startswith("k_stream_") and shape in ("small", "7Blayer"):
            # the passes over the weights, read from the trace: the wq|wk|wv launches in front of the attention entry, one per pass
            first = [e for e in trace[:trace.index(attn[0])] if e.startswith(want[0])]
            assert len(first) == (2 if family.endswith("/two-pass") else 1), (shape, wtype, n, family, trace[:trace.index(attn[0]) + 1])
    return family


_CLEAN = {}      # (shape, wtype, probe, n, past) -> (x_out, trace) of the clean call, kept for the non-finite twin of the case


def clean_call(product, shape, wtype, probe, n, past):
    key = (shape, wtype, probe, n, past)
    if key not in _CLEAN:
        _CLEAN[key] = run_call(product, get_probe(product, shape, wtype, probe), n, past)
    return _CLEAN[key]


def check_bound(product, shape, wtype, probe, n, past):
    P = get_probe(product, shape, wtype, probe)
    y, trace = clean_call(product, shape, wtype, probe, n, past)
    family = R.expected_route(shape, wtype, n, probe == "head")[0]
    rows = slice(past + n - 1, past + n) if probe == "head" else slice(past, past + n)
    ref = dict(out=P.ref["out"][rows], bound=P.ref["bound"][rows])
    br = R.ratio(y, ref)
    print(f"{probe} {shape} {wtype} n={n} past={past} [{family}]: error / bound {br:.4g}; {' '.join(dict.fromkeys(entry_name(e) for e in trace))}")
    check_route(trace, shape, wtype, n, probe == "head")
    r = REPORT.setdefault((probe, shape, wtype, family), [0.0, 0])
    r[0], r[1] = max(r[0], br), r[1] + 1
    err = np.abs(y.astype(np.float64) - ref["out"])
    bad = np.argwhere(~(err <= ref["bound"]))
    assert len(bad) == 0, (f"{probe} {shape} {wtype} n={n} past={past} [{family}]: {len(bad)} elements outside the bound, first (row, column) {bad[0].tolist()}: "
                           f"error {err[tuple(bad[0])]:.3e}, bound {ref['bound'][tuple(bad[0])]:.3e}; worst error / bound {br:.3g}")


def check_nan_row(product, shape, wtype, probe, n, past):
    P = get_probe(product, shape, wtype, probe)
    y, trace = clean_call(product, shape, wtype, probe, n, past)
    family = R.expected_route(shape, wtype, n)[0]
    y2, trace2 = run_call(product, P, n, past, nan_last=True)
    attn = " ".join(dict.fromkeys(e for e in trace if e.startswith(ATTN_ENTRIES)))
    assert [entry_name(e) for e in trace2] == [entry_name(e) for e in trace], (probe, shape, wtype, n, past)
    assert np.all(np.isfinite(y))
    changed = np.count_nonzero((y2[:n - 1].view(np.uint32) != y[:n - 1].view(np.uint32)).any(axis=1))
    assert y2[:n - 1].tobytes() == y[:n - 1].tobytes(), f"{probe} {shape} {wtype} n={n} past={past} [{family}; {attn}]: {changed} of rows 0..n-2 change when row n-1 is NaN"
    assert np.all(np.isnan(y2[n - 1])), f"{probe} {shape} {wtype} n={n} past={past} [{family}]: {np.count_nonzero(~np.isnan(y2[n - 1]))} elements of the NaN row are not NaN"


@pytest.mark.parametrize("shape,wtype,probe,n,past,check", CASES, ids=[f"{p}-{s}-{w}-n{n}-p{past}-{chk}" for s, w, p, n, past, chk in CASES])
def test_weight_launch(product, shape, wtype, probe, n, past, check):
    """check = bound: the route, and every element of every row inside the bound.
    check = nan: the same call with its last row all NaN - rows 0 .. n - 2 bit-identical to the clean call, row n - 1 NaN in every element.

    Every probe gives the NaN row a NaN V row (0 x NaN where wv = 0) and a NaN K row, so the twin also holds the attention kernel of the call to
    keeping a non-finite row out of the queries that do not see its key (csrc/kernels_attn.h: k_attn_flash takes a non-finite V value into its P V matrix
    product as 0 and adds it to the queries that do)."""
    t0 = time.time()
    try:
        (check_bound if check == "bound" else check_nan_row)(product, shape, wtype, probe, n, past)
    finally:
        TIMES[shape] = TIMES.get(shape, 0.0) + time.time() - t0


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------------
def crafted_blocks():
    """[(name, 32 float32 values)]: the edges of d = fl32(max|w| / 127), q = clamp(rint(fl32(w / d)), -127, 127), w' = fl32(d q), and the non-finite rule."""
    f = np.float32
    rng = np.random.default_rng(3)
    fmax = np.finfo(f).max
    sub = f(2.0 ** -149)
    blocks = [("zero", np.zeros(32, f)),
              ("negative-max", np.concatenate([[f(-3.0)], rng.uniform(-2.9, 2.9, 31).astype(f)])),
              ("ties", np.concatenate([[f(127.0)], (np.arange(31, dtype=f) - f(15)) + f(0.5)])),                       # d = 1 exactly: k + 0.5 goes to the even side
              ("ties-large", np.concatenate([[f(-127.0)], f(126.5) - f(2) * np.arange(31, dtype=f)])),
              ("subnormal", np.concatenate([[f(1e-40)], (rng.uniform(-1, 1, 31) * 1e-40).astype(f)])),                   # max / 127 is subnormal
              ("subnormal-least", np.concatenate([[sub], np.zeros(30, f), [-sub]])),                                     # max / 127 rounds to 0: q = 0
              ("subnormal-127", np.concatenate([[f(127) * sub], (np.arange(31, dtype=f) - f(15)) * sub])),              # d = the least subnormal, exact quotients
              ("flt-max", np.concatenate([[fmax, -fmax, fmax / f(2), np.nextafter(fmax, f(0))], (rng.uniform(-1, 1, 28) * fmax).astype(f)])),
              ("clamp-edge", np.concatenate([[f(127.0), f(126.5), np.nextafter(f(126.5), f(200)), f(-126.75), np.nextafter(f(127), f(0)), np.nextafter(f(-127), f(0))],
                                             rng.uniform(-127, 127, 26).astype(f)])),
              ("clamp-edge-inexact", np.concatenate([[f(1.0), np.nextafter(f(1), f(0)), -np.nextafter(f(1), f(0)), f(-1.0), f(253.0) / f(254.0)],
                                                     rng.uniform(-1, 1, 27).astype(f)])),
              ("nan", np.concatenate([[f(np.nan)], rng.uniform(-1, 1, 31).astype(f)])),
              ("nan-last-negative", np.concatenate([rng.uniform(-1, 1, 31).astype(f), [-f(np.nan)]])),
              ("inf", np.concatenate([[f(0.5), f(np.inf)], rng.uniform(-1, 1, 30).astype(f)])),
              ("neg-inf", np.concatenate([rng.uniform(-1, 1, 17).astype(f), [f(-np.inf)], rng.uniform(-1, 1, 14).astype(f)])),
              ("nan-and-inf", np.concatenate([[f(np.inf), f(np.nan), f(-np.inf)], np.zeros(29, f)]))]
    assert all(b.shape == (32,) and b.dtype == f for _, b in blocks)
    return blocks


def test_quantiser_matches_its_rule_bit_for_bit(product):
    """k_quantize_q8 on crafted 32-blocks set into a d x d matrix (Gaussian elsewhere), read back, against the numpy restatement of the rule in
    csrc/kernels_q8.h; a block that holds a NaN or an infinity dequantises to NaN in every element, and no other block does."""
    d = 256
    rng = np.random.default_rng(17)
    w = (rng.standard_normal((d, d)) / 16).astype(np.float32)
    blocks = crafted_blocks()
    where = {}
    for i, (name, b) in enumerate(blocks):                        # one per row, at a different block column each: the first, the last, in between
        row, col = 3 + 7 * i, (5 * i) % (d // 32)
        w[row, 32 * col:32 * col + 32] = b
        where[name] = (row, col)
    assert {c for _, c in where.values()} >= {0, d // 32 - 1}
    m = product.NewSyntheticModel(make_hparams(vocab=32, embd=d, mult=128, heads=2, layers=1, ctx=64), 3)
    try:
        m.SetTensor("layers.0.attention.wo.weight", w)
        m.QuantizeQ8()
        got = product.read(None, m.tensor("layers.0.attention.wo.weight")).reshape(d, d)
    finally:
        m.free()
    q, sc, want = R.quantize_q8(w)
    nonfinite = ~np.isfinite(w.reshape(d, d // 32, 32)).all(axis=2)
    assert nonfinite.sum() == 5 and np.array_equal(np.isnan(sc), nonfinite)
    for name, (row, col) in where.items():
        g, x = got[row, 32 * col:32 * col + 32], want[row, 32 * col:32 * col + 32]
        assert np.array_equal(np.isnan(g), np.isnan(x)), f"block {name}: NaN pattern {np.isnan(g).astype(int).tolist()}, the rule gives {np.isnan(x).astype(int).tolist()}; values {g.tolist()}"
        ok = np.isnan(x) | (g.view(np.uint32) == x.view(np.uint32))
        assert ok.all(), f"block {name}: elements {np.argwhere(~ok).ravel().tolist()} are {g[~ok].tolist()}, the rule gives {x[~ok].tolist()} (weights {w[row, 32 * col:32 * col + 32][~ok].tolist()})"
    assert np.array_equal(np.isnan(got), np.repeat(nonfinite, 32, axis=1)), "NaN outside the non-finite blocks, or a finite value inside one"
    fin = ~np.isnan(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32)), "the Gaussian rest of the matrix differs from the rule"
    # the rule's own edges, so that the crafted blocks are known to sit on them
    r, c = where["ties"]
    assert sc[r, c] == 1 and q[r, 32 * c + 1:32 * c + 32].tolist() == [int(np.rint(k + 0.5)) for k in range(-15, 16)] and 0 in q[r, 32 * c + 1:32 * c + 32].tolist()
    r, c = where["subnormal-least"]
    assert sc[r, c] == 0 and not np.any(q[r, 32 * c:32 * c + 32])
    r, c = where["subnormal"]
    assert 0 < sc[r, c] < np.finfo(np.float32).tiny and q[r, 32 * c] == 127
    r, c = where["flt-max"]
    # d = fl32(FLT_MAX / 127) is rounded UP, so the half lands below 63.5 and fl32(127 d) overflows: by the rule itself a weight of +-FLT_MAX (q = +-127)
    # comes back as +-inf - pinned here, the device and the rule agreeing bit for bit above; everything below 127 quanta stays finite
    assert q[r, 32 * c:32 * c + 4].tolist() == [127, -127, 63, 127] and sc[r, c] * np.float32(127) == np.inf
    assert np.array_equal(np.isinf(want[r, 32 * c:32 * c + 32]), np.abs(q[r, 32 * c:32 * c + 32]) == 127) and want[r, 32 * c + 1] == -np.inf
    r, c = where["clamp-edge"]
    assert q[r, 32 * c:32 * c + 6].tolist() == [127, 126, 127, -127, 127, -127]
    r, c = where["negative-max"]
    assert q[r, 32 * c] == -127 and sc[r, c] > 0


def test_zz_report():
    """Prints (and, with WEIGHT_PROBE_REPORT set, writes) the worst error / bound per (probe, shape, type, route family) of this session and the seconds
    each shape's tests took: the source of profiles/weight_probe.txt."""
    lines = [f"{p:5s} {s:10s} {w:4s} {fam:26s} calls {n:3d}   worst error/bound {br:.4f}" for (p, s, w, fam), (br, n) in sorted(REPORT.items())]
    lines += [f"seconds in the tests of {s}: {t:.1f}" for s, t in sorted(TIMES.items())]
    print("\n".join(lines))
    path = os.environ.get("WEIGHT_PROBE_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
