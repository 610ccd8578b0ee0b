"""f16 prompts of 65..128 tokens on k_stream_b9w_h (lh_ctx_set_f16_planes + lh_ctx_set_wide_planes, DESIGN 3k "Native wide planes kernel"): the synthetic
7B as fp32 and narrowed (Model.NarrowF16), both resident, one Eval of n tokens at past 0, four legs alternating in ONE process so that drift of the box
hits all alike:

  fp32 wide    the fp32 model with wide planes on: k_stream_b9w, eight bf16 products per weight
  f16 none     the f16 model with every switch off: each layer widened in front of k_stream_dma
  f16 stream   the f16 model with f16_stream on: k_stream_dma_h over the halves (the best f16 route before this kernel)
  f16 wide     the f16 model with f16_planes + wide_planes on (and f16_stream, for the rows they do not move): k_stream_b9w_h, six products per weight

A measurement is the mean over --evals back-to-back Evals (host clock around calls that end in a synchronisation; every Eval reads its logits back), taken
--repeats times per leg and length, the legs alternating; every context is warmed with every length first and held to the kernel its leg is named for.
No time is fixed in advance.  Recorded per length: every measurement, whether the SLOWEST f16-wide leg beats the FASTEST f16-stream leg, and the medians'
ratio to fp32 wide.  Per-launch times and the shader clock are not collected.  Writes what it measured to profiles/f16_wide_planes.txt (and prints it).
usage: python tools/bench_f16_wide.py [--shape 7B] [--layers 0] [--evals 20] [--repeats 5] [--note TEXT] [--out profiles/f16_wide_planes.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--evals", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--note", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_wide_planes.txt"))
args = ap.parse_args()

from llama_go_amd.mlapi import SHAPES, load_product, make_hparams, route_trace  # noqa: E402

CTX = 128
LENGTHS = (65, 80, 96, 112, 128)
LEGS = ("fp32 wide", "f16 none", "f16 stream", "f16 wide")
KERNEL = {"fp32 wide": "k_stream_b9w<", "f16 none": "k_stream_dma<", "f16 stream": "k_stream_dma_h<", "f16 wide": "k_stream_b9w_h<"}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def measure(c, toks):
    t0 = time.perf_counter()
    for _ in range(args.evals):
        c.Eval(toks, 0)
    return (time.perf_counter() - t0) / args.evals * 1e3


prod = load_product()
kw = dict(SHAPES[args.shape])
if args.layers:
    kw["layers"] = args.layers
hp = make_hparams(**kw, ctx=CTX)
m16 = prod.NewSyntheticModel(hp, 1234)
changed = m16.NarrowF16()
m32 = prod.NewSyntheticModel(hp, 1234)
ctxs = {"fp32 wide": m32.NewContext(CTX, 1), "f16 none": m16.NewContext(CTX, 1), "f16 stream": m16.NewContext(CTX, 1), "f16 wide": m16.NewContext(CTX, 1)}
ctxs["fp32 wide"].SetWidePlanes(True)
ctxs["f16 stream"].SetF16Stream(True)
ctxs["f16 wide"].SetF16Stream(True), ctxs["f16 wide"].SetF16Planes(True), ctxs["f16 wide"].SetWidePlanes(True)
toks = {n: [(31 * i + 5) % hp.vocabSize for i in range(n)] for n in LENGTHS}
for name, c in ctxs.items():           # warm every length on every leg; the legs must be on the kernels they are named for
    for n in LENGTHS:
        _, tr = route_trace(lambda: c.Eval(toks[n], 0))
        assert [k for k in KERNEL.values() if any(e.startswith(k) for e in tr)] == [KERNEL[name]], (name, n, tr)

say(f"# tools/bench_f16_wide.py --shape {args.shape} --layers {kw['layers']} --evals {args.evals} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {CTX}; fp32 as generated, f16 = NarrowF16 of the same seed ({changed} of its matrix elements rounded)")
say(f"# one Eval of n tokens at past 0, ms per Eval (mean of {args.evals} back to back); legs alternate in ONE process; host clock around calls that end in a synchronisation")
say("# per-launch times: not measured.  shader clock: not measured.")
if args.note:
    say(f"# {args.note}")
say()
wins = []
for n in LENGTHS:
    r = {name: [] for name in LEGS}
    for _ in range(args.repeats):
        for name in LEGS:
            r[name].append(measure(ctxs[name], toks[n]))
    med = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
    ok = max(r["f16 wide"]) < min(r["f16 stream"])
    wins.append((n, ok))
    say(f"  {n:3d} tokens   " + "   ".join(f"{k} {'  '.join(f'{x:7.3f}' for x in r[k])}" for k in LEGS))
    say(f"               medians " + "  ".join(f"{k} {med[k]:.3f}" for k in LEGS) + f"   f16 wide / fp32 wide {med['f16 wide'] / med['fp32 wide']:.3f} (MFMAs 6 / 8 = 0.750)   "
        f"slowest f16 wide {max(r['f16 wide']):.3f} vs fastest f16 stream {min(r['f16 stream']):.3f}: {'faster' if ok else 'NOT faster'}")
say()
say("slowest f16-wide leg beats the fastest f16-stream leg at: " + (", ".join(str(n) for n, ok in wins if ok) or "no length") +
    "; not at: " + (", ".join(str(n) for n, ok in wins if not ok) or "no length"))
for c in ctxs.values():
    c.free()
m32.free(); m16.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
