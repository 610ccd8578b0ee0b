"""The calls whose launch sequences tests/test_gpu_eval_routes.py pins, and the recorder of tests/golden/eval_route_traces.json.

Every case is one call into the plan's Eval (llama.go_amd/csrc/plan.hip, plan_eval) on a two-layer synthetic model, run under mlapi.route_trace: the
list of kernel instantiations it launched, in order.  The golden holds that list per case as recorded on an MI355X at the commit BEFORE plan_eval was
split into one function per route; the test requires the same lists of the code it runs against.

Recording (on the GPU machine, in a checkout of the commit to record; this file only needs what that commit's mlapi offers):
    python tests/eval_route_cases.py --record tests/golden/eval_route_traces.json
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CTX = 256
# Two layers everywhere a route has a reduce pass that writes the NEXT layer's norm rows (it exists only with a next layer).
SHAPES = {
    "small": dict(vocab=2048, embd=1024, mult=256, heads=8, layers=2),
    "7Bslice": dict(vocab=32000, embd=4096, mult=256, heads=32, layers=2),
    # tests/test_gpu_llama.py test_odd_shapes_match_oracle, third shape: 5 heads of 128, odd vocabulary, ff = 1712 - not a multiple of 32, so no grouped
    # MFMA launch takes it and every matrix goes through gemm_small_n / the column kernels.  (No shape of that test has an embd off the 128 grid; it is
    # the ff size that turns the tile routes away.)  A matrix of 1712 columns cannot be quantised, so this shape stays fp32 ...
    "odd640": dict(vocab=515, embd=640, mult=8, heads=5, layers=2),
    # ... and its twin of test_odd_shapes_block_int8 (ff = 1728: whole int8 blocks and GEMM tiles, but no k_stream_* launch) is built as both weight types:
    # block-int8 it takes the "n single steps" route up to 8 rows and the dequantising tile GEMM above.
    "odd640m32": dict(vocab=515, embd=640, mult=32, heads=5, layers=2),
    # k_skinny: the 65B layer shape (embd 8192, ff 22016) as one layer, which is how the suite reaches it (test_larger_shapes_slice_matches_oracle[65B], an
    # 8-token prompt): w1|w3 need 11 row tiles per workgroup, more than k_stream_* is built for, and 5..8 rows of 8192 columns have no k_gemv_rows launch
    # with the norm folded in.  The vocabulary is cut to 2048 rows: the lm_head's size decides neither of the two conditions.
    # (The route trace does not name k_skinny's own launches, nor the GEMV launches of the Step and Rows routes: these cases pin the attention entry
    # between them, and the suite's route log, tests/test_gpu_zz_routes.py, requires that k_skinny is still reached.)
    "65Blayer": dict(vocab=2048, embd=8192, mult=256, heads=64, layers=1),
}
MODELS = [("small", "f32"), ("small", "q8"), ("7Bslice", "f32"), ("7Bslice", "q8"), ("odd640", "f32"), ("odd640m32", "f32"), ("odd640m32", "q8"), ("65Blayer", "f32")]

EVAL_LENGTHS = {"f32": [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 112, 113, 128, 129, 192, 193],
                "q8": [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 64, 65, 88, 89, 128, 129]}
# one length per route, again behind 7 cached positions: the one-token step, the decode-stream rows, (block-int8) n single steps / the planes, (fp32) the
# folded-norm stream launch, the planes, the stream kernels, the two-pass prompt; the tile GEMM beyond
EVAL_LENGTHS_PAST7 = {"f32": [1, 4, 16, 64, 96, 129, 193], "q8": [1, 3, 5, 16, 128]}
BATCH_PODS = {"f32": [2, 4, 5, 8, 9, 16, 17, 48, 49, 64], "q8": [2, 3, 4, 5, 16, 64]}
VERIFY_ROWS = {"f32": 5, "q8": 4}    # (a verify pass carries what the decode stream carries: block-int8 stops at four rows)
STAGE_ROWS = [1, 4, 20, 60]
SKINNY_LENGTHS = [5, 8]              # the 65B layer: solo Evals only


def case_ids(shape, wtype):
    """The ids of a model's cases, in the order run_model runs them."""
    if shape == "65Blayer":
        return [f"eval_n{n}_past0" for n in SKINNY_LENGTHS] + [f"eval_n{SKINNY_LENGTHS[-1]}_past7"]
    ids = [f"eval_n{n}_past0" for n in EVAL_LENGTHS[wtype]] + [f"eval_n{n}_past7" for n in EVAL_LENGTHS_PAST7[wtype]]
    ids += [f"tick_pods{b}" for b in BATCH_PODS[wtype]]
    ids += [f"verify_n{VERIFY_ROWS[wtype]}"]
    ids += [f"stage_{which}_n{n}" for which in ("first", "last") for n in STAGE_ROWS]
    return ids


def _tokens(n, vocab, salt=0):
    return [(7 + 13 * i + 5 * salt) % vocab for i in range(n)]


def _traced(fn):
    """The trace of one call; a call the library refuses is pinned by its message."""
    from llama_go_amd.mlapi import MLError, route_trace
    try:
        return route_trace(fn)[1]
    except MLError as e:
        return [f"refused: {e}"]


def run_model(product, shape, wtype):
    """Builds the model and runs its cases -> {case id: [instantiation, ...]}."""
    import torch
    from llama_go_amd.mlapi import Batch, MLError, make_hparams
    kw = SHAPES[shape]
    hp = make_hparams(**kw, ctx=CTX)
    V, d, L = kw["vocab"], kw["embd"], kw["layers"]
    out = {}

    def build(layer0=0, layer1=0):
        m = product.NewSyntheticModel(hp, 4321, layer0, layer1)
        return m.QuantizeQ8() if wtype == "q8" else m

    m = build()
    try:
        c = m.NewContext(CTX, 1, False)
        try:
            for cid in [i for i in case_ids(shape, wtype) if i.startswith("eval_")]:
                n, past = int(cid.split("_")[1][1:]), int(cid.split("_")[2][4:])
                out[cid] = _traced(lambda: c.Eval(_tokens(n, V, past), past))
            if shape != "65Blayer":
                n = VERIFY_ROWS[wtype]
                out[f"verify_n{n}"] = _traced(lambda: c.Verify(_tokens(n, V, 3), 9))
        finally:
            c.free()
        for pods in ([] if shape == "65Blayer" else BATCH_PODS[wtype]):
            b = Batch(m, CTX, pods)
            try:
                b.Set(_tokens(pods, V, 1), [(3 * i) % 7 for i in range(pods)])
                out[f"tick_pods{pods}"] = _traced(b.Tick)
            finally:
                b.free()
    finally:
        m.free()
    if shape == "65Blayer":
        return out
    for which, (l0, l1) in (("first", (0, 1)), ("last", (L - 1, L))):
        sm = build(l0, l1)
        try:
            c = sm.NewContext(CTX, 1, False)
            try:
                x_in = torch.full((max(STAGE_ROWS), d), 0.25, dtype=torch.float32, device="cuda")
                x_out = torch.empty((max(STAGE_ROWS), d), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                for n in STAGE_ROWS:
                    toks = (C.c_uint32 * n)(*_tokens(n, V, 2)) if which == "first" else None

                    def stage():
                        if product.lib.llamago_Stage(c.h, toks, None, C.c_void_p(x_in.data_ptr()) if which == "last" else None,
                                                     C.c_void_p(x_out.data_ptr()) if which == "first" else None, n, 0, None, None):
                            raise MLError(product.last_error())
                    out[f"stage_{which}_n{n}"] = _traced(stage)
                assert product.lib.llamago_Sync(c.h) == 0, product.last_error()
            finally:
                c.free()
        finally:
            sm.free()
    return out


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def model_key(shape, wtype):
    return f"{shape}/{wtype}"


def record(path):
    from llama_go_amd.mlapi import load_product
    product = load_product()
    gold = {"num_cu": device_cus(), "traces": {}}
    for shape, wtype in MODELS:
        got = run_model(product, shape, wtype)
        assert list(got) and sorted(got) == sorted(case_ids(shape, wtype)), (shape, wtype, sorted(set(case_ids(shape, wtype)) ^ set(got)))
        gold["traces"][model_key(shape, wtype)] = {cid: " ".join(got[cid]) for cid in case_ids(shape, wtype)}
        print(f"{model_key(shape, wtype)}: {len(got)} cases, {sum(len(t) for t in got.values())} launches", flush=True)
    with open(path, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: eval_route_cases.py --record PATH")
    record(sys.argv[2])
