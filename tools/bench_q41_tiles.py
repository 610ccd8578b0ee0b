"""Q4_1 models on the bf16 tile GEMM of prompts beyond 128 rows (lh_ctx_set_q41_tiles, DESIGN 3m "Native tile GEMM"): a synthetic model as Q4_1
(Model.QuantizeQ41) and as its fp32 twin (QuantizeQ41 + ExpandQ41), both resident, three legs alternating in ONE process so that drift of the box hits all alike:

  fp32      the twin: k_gemm_b9 over fp32 weights
  q41 off   the Q4_1 model with the switch off: every layer expanded into an fp32 image (seven k_expand_q41 passes) in front of the same launches
  q41 on    the Q4_1 model with the switch on: k_gemm_b9_q41 reads the nibble and (d, m) planes (no expansion pass but the logits row's output matrix)

One Eval of 193 / 256 / 512 / 1024 tokens at past 0 that computes the last row's logits, ms (best of 3 per leg and repeat; every leg warmed by one Eval).
No speed is promised: the ratios on / off and on / fp32 are reported as they come out, with the spread (min .. max over the repeats) of every leg.  Appends what
it measured to the output file (and prints it), so that the runs of one measurement (a probe build of another ring depth: make EXTRA=-DB9Q41_NST=4) stand in one file.
usage: python tools/bench_q41_tiles.py [--shape 7B] [--layers 0] [--lengths 193,256,512,1024] [--repeats 3] [--note TEXT] [--out profiles/q41_tiles.txt] [--fresh]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--lengths", default="193,256,512,1024")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--note", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q41_tiles.txt"))
ap.add_argument("--fresh", action="store_true", help="truncate the output file instead of appending to it")
args = ap.parse_args()

from llama_go_amd.mlapi import SHAPES, load_product, make_hparams, route_trace  # noqa: E402

LENGTHS = tuple(int(x) for x in args.lengths.split(","))
PCTX = max(LENGTHS) + 1
LEGS = ("fp32", "q41 off", "q41 on")


def tokens(m, n):
    return [(31 * i + 5) % m.hp.vocabSize for i in range(n)]


def prompt_leg(m, on, n):
    c = m.NewContext(PCTX, 1)
    c.SetQ41Tiles(on)
    toks = tokens(m, n)
    c.Eval(toks, 0)                                                    # warm
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        c.Eval(toks, 0)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    c.free()
    return best * 1e3


def tile_launches(m, on, n):
    c = m.NewContext(PCTX, 1)
    c.SetQ41Tiles(on)
    _, tr = route_trace(lambda: c.Eval(tokens(m, n), 0))
    c.free()
    fam = [e.split("<")[0] for e in tr]
    return {k: fam.count(k) for k in ("k_gemm_b9", "k_gemm_b9_q41", "k_gemm_glds", "k_expand_q41")}, sorted({e for e in tr if e.startswith("k_gemm_")})


lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


prod = load_product()
kw = dict(SHAPES[args.shape])
if args.layers:
    kw["layers"] = args.layers
hp = make_hparams(**kw, ctx=PCTX)
mq = prod.NewSyntheticModel(hp, 1234).QuantizeQ41()
mf = prod.NewSyntheticModel(hp, 1234).QuantizeQ41().ExpandQ41()
legs = (("fp32", mf, False), ("q41 off", mq, False), ("q41 on", mq, True))
say(f"# tools/bench_q41_tiles.py --shape {args.shape} --layers {kw['layers']} --lengths {args.lengths} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {PCTX}; q41 = QuantizeQ41, fp32 = ExpandQ41 of the same blocks")
say("# legs alternate in ONE process; host clock around an Eval that ends in a synchronisation")
if args.note:
    say(f"# {args.note}")
for name, m, on in legs:
    counts, insts = tile_launches(m, on, LENGTHS[0])
    say(f"# {name:8s} at {LENGTHS[0]} tokens: {counts}  {' '.join(insts)}")
say()

say("one Eval of n tokens at past 0, ms: median (min .. max) over the repeats, each the best of 3")
for n in LENGTHS:
    r = {name: [] for name in LEGS}
    for _ in range(args.repeats):
        for name, m, on in legs:
            r[name].append(prompt_leg(m, on, n))
    med = {name: sorted(r[name])[len(r[name]) // 2] for name in LEGS}
    say(f"  {n:4d} tokens   " + "   ".join(f"{name} {med[name]:8.3f} ({min(r[name]):.3f} .. {max(r[name]):.3f})" for name in LEGS) +
        f"   on / off {med['q41 on'] / med['q41 off']:.3f}  on / fp32 {med['q41 on'] / med['fp32']:.3f}  "
        f"slowest on {max(r['q41 on']):.3f} vs fastest off {min(r['q41 off']):.3f}: {'faster' if max(r['q41 on']) < min(r['q41 off']) else 'NOT faster'}")
say()
mf.free(); mq.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w" if args.fresh else "a") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
