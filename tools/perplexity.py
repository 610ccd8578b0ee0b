"""Perplexity of a token sequence under a model on the MI355X, fp32 and (--int8 / --int4) the same model after QuantizeQ8 / QuantizeQ4: the log-probs are reduced on
the device (lh_llama_score), only 32 bytes per token come back.  The project has no tokenizer: token ids come from a .npy (--ids), from a
seeded generator (--random N) or, by default, from the committed golden run (the 8-token prompt + the 100 ids the checker decoded).
Convention (include/llamago_ext.h, llamago_Perplexity): windows of --ctx tokens, each from position 0 in Evals of at most --chunk rows,
row i against token i+1, a window's last row not scored.  Prints one JSON line; `ms` = wall time of the whole scored pass (median of --reps,
after one warm-up pass), `probe_gbps` (--probe) = what a bare read of one chunk's [rows][vocab] logits reaches on this box.
On synthetic (random) weights the figures say little about real models: they exercise the path and compare the two weight formats.
usage: python tools/perplexity.py (--model file.bin | --synthetic) [--shape 7B] [--layers L] [--ctx 1024] [--chunk 512] [--ids ids.npy | --random N] [--int8] [--int4]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, hbm_read_probe, load_product, make_hparams  # noqa: E402

ap = argparse.ArgumentParser()
src = ap.add_mutually_exclusive_group(required=True)
src.add_argument("--model", help="a ggjt file")
src.add_argument("--synthetic", action="store_true", help="synthetic weights, seed 1234")
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0, help="synthetic: truncate the shape to this many layers")
ap.add_argument("--ctx", type=int, default=1024)
ap.add_argument("--chunk", type=int, default=0, help="rows per Eval (0: 512)")
ap.add_argument("--ids", help=".npy of token ids")
ap.add_argument("--random", type=int, default=0, help="this many seeded random ids instead of the golden sequence")
ap.add_argument("--int8", action="store_true", help="also the same model after QuantizeQ8, and the difference")
ap.add_argument("--int4", action="store_true", help="also the same model after QuantizeQ4 (block-int4), and the difference")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--probe", action="store_true")
args = ap.parse_args()

prod = load_product()


def load_model():
    if args.model:
        return prod.LoadModel(args.model, args.ctx)
    kw = dict(SHAPES[args.shape])
    if args.layers:
        kw["layers"] = args.layers
    return prod.NewSyntheticModel(make_hparams(**kw, ctx=args.ctx), 1234)


def run(wtype):
    m = load_model()
    if wtype == 7:
        m.QuantizeQ8()
    if wtype == 2:
        m.QuantizeQ4()
    V = m.hp.vocabSize
    if args.ids:
        ids = [int(t) for t in np.load(args.ids).ravel()]
    elif args.random:
        ids = [int(t) for t in np.random.default_rng(0).integers(0, V, args.random)]
    else:
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "7b_seed1234_ids.json")))
        ids = [t for t in PROMPT + gold["ids"] if t < V]
    c = m.NewContext(args.ctx, 1)
    nll, cnt = c.Perplexity(ids, args.chunk)             # warm-up: scratch, kernel attributes
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        nll, cnt = c.Perplexity(ids, args.chunk)
        ts.append(time.perf_counter() - t0)
    c.free()
    m.free()
    return {"nll_sum": nll, "n_scored": cnt, "perplexity": math.exp(nll / cnt) if cnt else None, "ms": round(sorted(ts)[len(ts) // 2] * 1e3, 3)}, len(ids), V


out = {"model": args.model or f"synthetic {args.shape}" + (f" x{args.layers} layers" if args.layers else ""), "ctx": args.ctx, "chunk": args.chunk or 512}
out["fp32"], out["n_tokens"], V = run(0)
if args.int4:
    out["int4"], _, _ = run(2)
    out["perplexity_int4_minus_fp32"] = out["int4"]["perplexity"] - out["fp32"]["perplexity"]
    out["nll_per_token_int4_minus_fp32"] = out["int4"]["nll_sum"] / out["int4"]["n_scored"] - out["fp32"]["nll_sum"] / out["fp32"]["n_scored"]
if args.int8:
    out["int8"], _, _ = run(7)
    out["perplexity_int8_minus_fp32"] = out["int8"]["perplexity"] - out["fp32"]["perplexity"]
    out["nll_per_token_int8_minus_fp32"] = out["int8"]["nll_sum"] / out["int8"]["n_scored"] - out["fp32"]["nll_sum"] / out["fp32"]["n_scored"]
if args.probe:
    rows = min(out["chunk"], args.ctx, out["n_tokens"])
    out["probe_bytes"] = rows * V * 4
    out["probe_gbps"] = round(hbm_read_probe(prod, rows * V * 4, 20), 1)
if args.synthetic:
    out["note"] = "synthetic weights: says little about real models"
print(json.dumps(out))
