"""Every attention kernel of the fused plan against a float64 reference, row by row (tests/attention_ref.py: the probe layer, the bound, the case matrix).

A probe layer (attention_norm = ffn_norm = 1, wq = a I, wk = b I, wv = wo = I, w1 = w2 = w3 = 0; llamago_SetModelTensor) makes x_out = x_in + attention(x_in),
so a middle pipeline stage (llamago_Stage -> plan_eval) shows EVERY row of the attention output.  Per case: the calls that feed one sequence to a context;
every checked call must
  * launch exactly the attention kernels the case names (route trace, include/llamahip.h),
  * keep every element of every row inside the bound computed from the operands,
  * keep its error E (in units of the rounding floor) within K_SPREAD x the E of a plain float32 numpy evaluation,
with the regime's defining property asserted on the reference first.  fp32 and block-int8 weights (the reference then takes the dequantised weights read
back from the device).  Whole one-layer models (output = I, vocab = d) carry the same layer through plain Eval (captured decode graph, device-side `past`) and
through lh_batch (every pod's row at its own position of its own cache).  The stale-row cases require bit-identical results on a cache that held decoy rows,
then NaN rows, before the sequence restarts at position 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R   # noqa: E402
from llama_go_amd.mlapi import Batch, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.case_matrix()
WTYPES = ("f32", "q8")
ATTN_ENTRIES = ("k_attention", "k_attn_flash", "attention_gemm", "k_softmax_causal", "k_transpose_v")
REPORT = {}    # route family -> [worst error / bound, worst E(hip) / E(float32), calls]


def attention_entries(trace):
    return [e for e in trace if e.startswith(ATTN_ENTRIES)]


_MODELS = {}


def probe_model(product, H, hd, a, b, wtype, whole=False, emb=None):
    """The probe layer as a middle pipeline stage (layers [1, 2) of 3), or as a whole one-layer model with tok_embeddings = emb, norm = 1, output = I.
    Returns (model, weights read back from the device as float64).  Stage models are kept for the session (a few hundred KB each)."""
    key = (H, hd, a, b, wtype)
    if not whole and key in _MODELS:
        return _MODELS[key]
    d = H * hd
    hp = make_hparams(vocab=d if whole else 32, embd=d, mult=128, heads=H, layers=1 if whole else 3, ctx=64)
    m = product.NewSyntheticModel(hp, 7, 0 if whole else 1, 1 if whole else 2)
    L = "layers.0." if whole else "layers.1."
    eye, F = np.eye(d, dtype=np.float32), m.ffSize
    m.SetTensor(L + "attention_norm.weight", np.ones(d))
    m.SetTensor(L + "ffn_norm.weight", np.ones(d))
    m.SetTensor(L + "attention.wq.weight", np.float32(a) * eye)
    m.SetTensor(L + "attention.wk.weight", np.float32(b) * eye)
    m.SetTensor(L + "attention.wv.weight", eye)
    m.SetTensor(L + "attention.wo.weight", eye)
    for w, shape in (("w1", (F, d)), ("w3", (F, d)), ("w2", (d, F))):
        m.SetTensor(L + f"feed_forward.{w}.weight", np.zeros(shape))
    if whole:
        m.SetTensor("norm.weight", np.ones(d))
        m.SetTensor("output.weight", eye)
        m.SetTensor("tok_embeddings.weight", emb)
    if wtype == "q8":
        m.QuantizeQ8()
    rd = lambda n: product.read(None, m.tensor(n)).astype(np.float64)   # noqa: E731
    W = dict(attn_norm=rd(L + "attention_norm.weight").reshape(d), wq=rd(L + "attention.wq.weight").reshape(d, d), wk=rd(L + "attention.wk.weight").reshape(d, d),
             wv=rd(L + "attention.wv.weight").reshape(d, d), wo=rd(L + "attention.wo.weight").reshape(d, d))
    assert np.all(rd(L + "ffn_norm.weight") == 1) and all(np.all(rd(L + f"feed_forward.{w}.weight") == 0) for w in ("w1", "w2", "w3")), "the FFN of the probe must add exactly 0"
    if whole:
        W.update(norm=rd("norm.weight").reshape(d), output=rd("output.weight").reshape(d, d))
    for n in ("wq", "wk", "wv", "wo"):
        assert np.count_nonzero(W[n] - np.diag(np.diag(W[n]))) == 0, n
    if not whole:
        _MODELS[key] = (m, W)
    return m, W


def run_stage_calls(product, model, ctx_size, d, steps, X, prefill=()):
    """Feeds the rows of X to a fresh context in `steps` [(n, past, checked)] through llamago_Stage; prefill: whole-window inputs evaluated at position 0
    first (stale-row cases).  -> (x_out [T][d] with NaN in rows no checked call wrote, {past: trace} of the checked calls)."""
    import torch
    c = model.NewContext(ctx_size, 1, False)
    try:
        T = X.shape[0]
        xin = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        xout = torch.full((max(T, ctx_size), d), float("nan"), dtype=torch.float32, device="cuda")
        scratch = torch.empty((ctx_size, d), dtype=torch.float32, device="cuda")
        pre = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).cuda() for p in prefill]
        torch.cuda.synchronize()

        def stage(src, dst, n, past):
            rc = product.lib.llamago_Stage(c.h, None, None, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, past, None, None)
            assert rc == 0, product.last_error()
            return rc

        for p in pre:
            stage(p, scratch, ctx_size, 0)
        traces = {}
        for n, past, checked in steps:
            if checked:
                _, tr = route_trace(lambda: stage(xin[past], xout[past], n, past))
                traces[past] = tr
            else:
                stage(xin[past], scratch, n, past)
        assert product.lib.llamago_Sync(c.h) == 0, product.last_error()
        return xout[:T].cpu().numpy(), traces
    finally:
        c.free()


def expect_route(case, n, trace):
    got = attention_entries(trace)
    want = case.route.split()
    if want[0].startswith("attention_gemm"):
        assert got == [want[0], "k_softmax_causal", "k_transpose_v"], (case, got)
        i = trace.index(want[0])
        assert len(trace) >= i + 5 and trace[i + 1].startswith("k_gemm_") and "<2,2,2,2>" in trace[i + 1] and trace[i + 2:i + 4] == ["k_softmax_causal", "k_transpose_v"] \
            and trace[i + 4].startswith("k_gemm_") and "<2,2,2,1>" in trace[i + 4], (case, trace[i:i + 5])
    else:
        assert got == want, (case, n, got, want)


def judge(case, wtype, y, ref, ref32, family):
    """Both assertions on the rows of one checked call (y, ref, ref32 already cut to them); the figures go to REPORT first."""
    br, e_hip, e_32 = R.bound_ratio(y, ref), R.case_error(y, ref), R.case_error(ref32, ref)
    r = REPORT.setdefault((family, wtype), [0.0, 0.0, 0])
    r[0], r[1], r[2] = max(r[0], br), max(r[1], e_hip / e_32), r[2] + 1
    err = np.abs(y - ref["out"])
    bad = np.argwhere(~(err <= ref["bound"]))
    assert len(bad) == 0, f"{case} {wtype}: {len(bad)} elements outside the bound, first (row, column) {bad[0]}: error {err[tuple(bad[0])]:.3e}, bound {ref['bound'][tuple(bad[0])]:.3e}; worst error / bound {br:.3g}"
    assert e_hip <= R.K_SPREAD * e_32, f"{case} {wtype}: error {e_hip:.1f} floors, the float32 evaluation's {e_32:.1f}: more than {R.K_SPREAD} x"


def cut(ref, sel):
    return dict(out=ref["out"][sel], bound=ref["bound"][sel], floor=ref["floor"][sel])


def real_slots():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_attention_rows_within_bound(product, case, wtype):
    if case.name.startswith("cut-"):     # the part boundaries the keys sit on were computed for 512 workgroup slots: hold on this device too
        n, past = case.calls[0]
        assert R.flash_parts(n, past, case.H, real_slots()) == R.flash_parts(n, past, case.H, 512), "work list differs on this device: rebuild the cut cases for its CU count"
    model, W = probe_model(product, case.H, case.hd, case.a, case.b, wtype)
    X, rows, steps = case.sequence(), case.checked_rows(), case.steps()
    ref = R.reference(X, W, case.H, rows)
    R.check_regime(case, ref, rows)
    ref32 = R.f32_textbook(X, W, case.H, rows)
    y, traces = run_stage_calls(product, model, case.ctx, case.d, steps, X)
    family = case.route.split("/")[0]
    for n, past, checked in steps:
        if checked:
            expect_route(case, n, traces[past])
            # the prompt attention's call site in eval_planes (layers over activation planes): block-int8 at 5..64 rows, fp32 at 49..64
            if wtype == "q8" and 5 <= n <= 64:
                assert any(e.startswith("k_stream_q8b") for e in traces[past]), (case, "block-int8 rows must take eval_planes", traces[past])
            if wtype == "f32" and 49 <= n <= 64:
                assert any(e.startswith("k_stream_b9") for e in traces[past]), (case, "fp32 at 49..64 rows must take eval_planes", traces[past])
    # the case as a whole - all rows of all its checked calls - as K_SPREAD was measured (tests/test_attention_bound_cpu.py)
    yc = y[rows].astype(np.float64)
    print(f"{case.name} {wtype}: error / bound {R.bound_ratio(yc, ref):.4g}, E(hip) {R.case_error(yc, ref):.2f}, E(float32) {R.case_error(ref32, ref):.2f}; "
          f"{' '.join(attention_entries(traces[steps[-1][1]]))}")
    judge(case, wtype, yc, ref, ref32, family)


STALE = [c for c in CASES if c.name in (
    "dec-hd128-T65-onehot-first", "dec-hd64-T65-ramp", "dec-hd32-T129-offset", "dec-hd256-T65-tie", "rows8-p40-onehot-past", "rows31-p40-ramp", "split320-tie-chunks",
    "split1152-onehot-c8first", "flash-n64-p37-onehot-past", "flash-n97-p31-tie-tiles", "cut-n64-p1920-tie-parts", "cut-n700-p0-ramp", "gemm-hd32-n70-p21-tie", "gemm-hd64-n130-p0-ramp")]


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("case", STALE, ids=lambda c: c.name)
def test_stale_cache_rows_change_nothing(product, case, wtype):
    """The cache state behind a context swap: the window once full of decoy rows (they would win every query and carry values 200 x the usual ones), then of
    NaN rows, then the sequence restarts at position 0.  Bit-identical to the run on a fresh context, on every route.  (Ordinary NaN arithmetic in rows the
    mask excludes; nothing here is out of bounds.)"""
    model, W = probe_model(product, case.H, case.hd, case.a, case.b, wtype)
    X, steps = case.sequence(), case.steps()
    fresh, tr0 = run_stage_calls(product, model, case.ctx, case.d, steps, X)
    decoy = R.decoy_rows(case.ctx, case.H, case.hd)
    stale, tr1 = run_stage_calls(product, model, case.ctx, case.d, steps, X, prefill=(decoy, np.full((case.ctx, case.d), np.nan, dtype=np.float32)))
    rows = case.checked_rows()
    assert len(STALE) == 14
    assert np.all(np.isfinite(fresh[rows])), case
    assert {k: attention_entries(v) for k, v in tr0.items()} == {k: attention_entries(v) for k, v in tr1.items()}
    assert fresh[rows].tobytes() == stale[rows].tobytes(), f"{case} {wtype}: {np.count_nonzero(fresh[rows] != stale[rows])} elements differ behind stale cache rows"


# ---- whole models: plain Eval (the contract route) and lh_batch -----------------------------------------------------------------------------
def whole_weights_case(name, H, hd, T, regime, g, keys=()):
    return R.Case(name, "", H, hd, 0, calls=[(T, 0)], regime=regime, g=g, keys=keys)


EVAL_CASES = [("eval-ctx256-onehot", 2, 128, 256, "k_attention/hd128/n1", "onehot", -R.G_STRONG, (39,)),
              ("eval-ctx256-ramp", 2, 128, 256, "k_attention/hd128/n1", "ramp", 60.0, ()),
              ("eval-ctx320-tie", 2, 128, 320, "k_attention_split/c3/n1 k_attention_combine/c3/n1", "tie", -R.G_STRONG, (3, 38)),
              ("eval-ctx320-offset", 2, 128, 320, "k_attention_split/c3/n1 k_attention_combine/c3/n1", "offset", -R.G_STRONG, ())]


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("spec", EVAL_CASES, ids=lambda s: s[0])
def test_solo_decode_through_eval(product, spec, wtype):
    """llama.Eval of a 40-token prompt and eight one-token Evals on a whole probe model: the decode steps run as the captured graph (the route is traced once,
    while it is captured; the replays launch nothing new) with `past` read on the device.  Token t is row t of the sequence; the logits are
    output (RMSNorm(x_out) * norm) = x_out / rms(x_out)."""
    name, H, hd, ctx, route, regime, g, keys = spec
    T0, steps_n = 40, 8
    case = whole_weights_case(name, H, hd, T0 + steps_n, regime, g, keys)
    X = case.sequence()
    d = case.d
    emb = np.zeros((d, d), dtype=np.float32)
    emb[:case.T] = X
    DECOY, NAN = 200, 201                          # token ids of a decoy row and of a NaN row (no prompt uses them)
    emb[DECOY], emb[NAN] = R.decoy_rows(1, H, hd)[0], np.nan
    model, W = probe_model(product, H, hd, case.a, case.b, wtype, whole=True, emb=emb)
    c = model.NewContext(ctx, 1, False)
    c2 = model.NewContext(ctx, 1, False)
    try:
        rows = np.arange(T0 - 1, case.T)
        ref = R.reference(X, W, H, rows)
        R.check_regime(case, ref, rows)
        refl = R.through_final_norm(ref, W)
        ref32 = R.f32_final_norm(R.f32_textbook(X, W, H, rows), W)
        got, traces = [], []
        lg, tr = route_trace(lambda: c.Eval(list(range(T0)), 0))
        got.append(lg)
        traces.append(attention_entries(tr))
        for s in range(steps_n):
            lg, tr = route_trace(lambda: c.Eval([T0 + s], T0 + s))
            assert product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h)) == 1
            got.append(lg)
            traces.append(attention_entries(tr))
        assert traces[0] == ["k_attn_flash/uncut/p1"], traces[0]
        assert traces[1] == route.split(), traces[1]                    # traced while the decode graph is captured ...
        assert all(t == [] for t in traces[2:]), traces[2:]             # ... and replayed from then on
        y = np.stack(got).astype(np.float64)
        print(f"{name} {wtype}: error / bound {R.bound_ratio(y, refl):.4g}, E(hip) {R.case_error(y, refl):.2f}, E(float32) {R.case_error(ref32, refl):.2f}")
        judge(case, wtype, y, cut(refl, slice(None)), ref32, "eval:" + route.split("/")[0])
        # the same Evals on a context whose window held decoy rows, then NaN rows (the cache state behind a context swap): not one bit differs
        c2.Eval([DECOY] * ctx, 0)
        c2.Eval([NAN] * ctx, 0)
        again = [c2.Eval(list(range(T0)), 0)] + [c2.Eval([T0 + s], T0 + s) for s in range(steps_n)]
        assert np.stack(again).tobytes() == np.stack(got).tobytes(), f"{name} {wtype}: logits differ behind stale cache rows"
    finally:
        c.free()
        c2.free()
        model.free()


BATCH_CASES = [("batch-ctx256-5pods", 4, 128, 256, (1, 2, 127, 128, 255), "k_attention/rows/hd128/n5"),
               ("batch-ctx256-12pods", 4, 128, 256, (1, 2, 127, 128, 255, 3, 63, 64, 65, 200, 31, 32), "k_attention/rows/hd128/n12"),
               ("batch-ctx384-5pods", 4, 128, 384, (1, 2, 127, 128, 383), "k_attention_split/rows/c3/n5 k_attention_combine/c3/n5"),
               ("batch-ctx384-9pods", 4, 128, 384, (1, 2, 127, 128, 383, 129, 256, 257, 300), "k_attention_split/rows/c3/n9 k_attention_combine/c3/n9")]


@pytest.mark.parametrize("wtype", WTYPES)
@pytest.mark.parametrize("regime", ("onehot", "offset"))
@pytest.mark.parametrize("spec", BATCH_CASES, ids=lambda s: s[0])
def test_batch_rows_within_bound(product, spec, regime, wtype):
    """lh_batch: every pod evaluates its prompt (tokens 0..L-1 = rows 0..L-1 of the sequence), then ONE tick takes every pod's next token at position L of its
    own cache - positions 1, 2, 127, 128 and ctx - 1 side by side (a tick at position 0 does not exist: test_batch_refuses_an_empty_prompt).  The tick's
    token is the greedy id of the prompt's last row, so the vocabulary IS the sequence (d rows: whatever id comes, it is a row of the regime) and the reference
    is built per pod from the ids the batch returns.  Every pod's logits row is judged, with the regime asserted on its reference first: one-hot on key 0
    (whatever row asks), or the common offset.  Then the same run on a batch whose caches held decoy rows and then NaN rows: bit-identical."""
    name, H, hd, ctx, lens, route = spec
    d = H * hd
    DECOY, NAN = 400, 401                         # token ids of a decoy row and of a NaN row: beyond every prompt, and value columns no argmax picks
    assert max(lens) + 1 <= ctx <= DECOY < d
    case = whole_weights_case(f"{name}-{regime}", H, hd, d, regime, -R.G_STRONG, (0,) if regime == "onehot" else ())
    emb = case.sequence().copy()
    emb[DECOY], emb[NAN] = R.decoy_rows(1, H, hd)[0], np.nan
    model, W = probe_model(product, H, hd, case.a, case.b, wtype, whole=True, emb=emb)
    b = Batch(model, ctx, len(lens))
    b2 = Batch(model, ctx, len(lens))
    try:
        assert b.batched
        prompts = [list(range(L)) for L in lens]
        (ids, lg), tr = route_trace(lambda: b.GreedyDecode(prompts, 2, want_logits=True))
        got = attention_entries(tr)
        assert got[-len(route.split()):] == route.split(), (name, got)
        assert [e for e in got if "/rows/" in e] == [e for e in route.split() if "/rows/" in e], (name, got)   # one tick, one rows launch
        ys, refs, r32 = [], [], []
        for i, L in enumerate(lens):
            assert ids[i][0] not in (0, DECOY, NAN), (name, i, ids[i])
            Xi = np.concatenate([emb[:L], emb[ids[i][0]][None, :]])
            ref0 = R.reference(Xi, W, H, [L])
            assert R.check_regime(case, ref0, np.array([L])) > 0, (name, i, L)
            refs.append(R.through_final_norm(ref0, W))
            r32.append(R.f32_final_norm(R.f32_textbook(Xi, W, H, [L]), W))
            ys.append(lg[i])
        ref = {k: np.concatenate([r[k] for r in refs]) for k in ("out", "bound", "floor")}
        y = np.stack(ys).astype(np.float64)
        print(f"{name} {regime} {wtype}: error / bound {R.bound_ratio(y, ref):.4g}, E(hip) {R.case_error(y, ref):.2f}, E(float32) {R.case_error(np.concatenate(r32), ref):.2f}")
        judge(case, wtype, y, ref, np.concatenate(r32), "batch:" + route.split("/")[0])
        b2.Prompt([[DECOY] * ctx for _ in lens])
        b2.Prompt([[NAN] * ctx for _ in lens])
        ids2, lg2 = b2.GreedyDecode(prompts, 2, want_logits=True)
        assert ids2 == ids and lg2.tobytes() == lg.tobytes(), f"{name} {regime} {wtype}: the tick differs behind stale cache rows"
    finally:
        b.free()
        b2.free()
        model.free()


def test_batch_refuses_an_empty_prompt(product):
    """A pod's tick at position 0 would need an empty prompt: refused, with the documented message."""
    from llama_go_amd.mlapi import MLError
    m = product.NewSyntheticModel(make_hparams(vocab=128, embd=128, mult=128, heads=1, layers=1, ctx=64), 3)
    b = Batch(m, 64, 2)
    try:
        with pytest.raises(MLError, match=r"prompt of 0 tokens outside 1\.\.64"):
            b.Prompt([[1, 2], []])
    finally:
        b.free()
        m.free()


def test_set_model_tensor_fails_loudly(product):
    from llama_go_amd.mlapi import MLError
    hp = make_hparams(vocab=32, embd=128, mult=128, heads=1, layers=1, ctx=64)
    m = product.NewSyntheticModel(hp, 3)
    try:
        one = np.ones(128, dtype=np.float32)
        m.SetTensor("norm.weight", 2 * one)
        assert np.all(product.read(None, m.tensor("norm.weight")) == 2)
        with pytest.raises(MLError, match="no tensor"):
            m.SetTensor("layers.7.attention.wq.weight", one)
        with pytest.raises(MLError, match="elements"):
            m.SetTensor("norm.weight", np.ones(127))
        c = m.NewContext(64, 1, False)
        with pytest.raises(MLError, match="alive"):
            m.SetTensor("norm.weight", one)
        c.free()
        m.SetTensor("norm.weight", one)
        m.QuantizeQ8()
        with pytest.raises(MLError, match="quantised"):
            m.SetTensor("output.weight", np.zeros((32, 128)))
        m.SetTensor("norm.weight", one)          # (norm vectors stay fp32)
    finally:
        m.free()


def test_zz_report():
    """Prints (and, with ATTENTION_BOUND_REPORT set, writes) the worst figures per route of this session: the source of profiles/attention_bound.txt."""
    lines = [f"{fam:28s} {wt:4s} calls {n:5d}   worst error/bound {br:.4f}   worst E(hip)/E(float32) {er:.3f}" for (fam, wt), (br, er, n) in sorted(REPORT.items())]
    print("\n".join(lines))
    path = os.environ.get("ATTENTION_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    for _, (m, _) in list(_MODELS.items()):
        m.free()
    _MODELS.clear()
