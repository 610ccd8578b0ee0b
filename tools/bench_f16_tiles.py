"""f16 models on the bf16 tile GEMM of prompts beyond 128 rows (lh_ctx_set_f16_tiles, DESIGN 3k "Native tile GEMM"): a synthetic model as fp32 and narrowed
(Model.NarrowF16), both resident, three legs alternating in ONE process so that drift of the box hits all alike:

  fp32      the fp32 model: k_gemm_b9 (eight bf16 products) over fp32 weights
  f16 off   the f16 model with the switch off: every layer widened into an fp32 image (seven k_widen_f16 passes) in front of the same k_gemm_b9 launches
  f16 on    the f16 model with the switch on: k_gemm_b9_h reads the halves (six products, no widening pass)

One Eval of 193 / 256 / 512 / 1024 tokens at past 0 that computes the last row's logits, ms (best of 3 per leg and repeat).

Condition the route ships under (not a target): at every measured length the slowest f16-on leg is faster than the fastest f16-off leg - off does
strictly more work.  on / fp32 is reported whatever it is.  Appends what it measured to the output file (and prints it), so that the runs of one
measurement (7B, 13B, a probe build of another ring depth) stand in one file.
usage: python tools/bench_f16_tiles.py [--shape 7B] [--layers 0] [--lengths 193,256,512,1024] [--repeats 3] [--note TEXT] [--out profiles/f16_tiles.txt] [--fresh]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_tiles.txt"))
ap.add_argument("--fresh", action="store_true", help="truncate the output file instead of appending to it")
args = ap.parse_args()

from llama_go_amd.mlapi import SHAPES, load_product, make_hparams, route_trace  # noqa: E402

LENGTHS = tuple(int(x) for x in args.lengths.split(","))
PCTX = max(LENGTHS) + 1
LEGS = ("fp32", "f16 off", "f16 on")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def prompt_leg(m, on, n):
    c = m.NewContext(PCTX, 1)
    c.SetF16Tiles(on)
    toks = [(31 * i + 5) % m.hp.vocabSize for i in range(n)]
    c.Eval(toks, 0)                                                    # warm
    best = min(timed(lambda: c.Eval(toks, 0))[1] for _ in range(3))
    c.free()
    return best * 1e3


def tile_launches(m, on, n):
    c = m.NewContext(PCTX, 1)
    c.SetF16Tiles(on)
    _, tr = route_trace(lambda: c.Eval([(31 * i + 5) % m.hp.vocabSize for i in range(n)], 0))
    c.free()
    fam = [e.split("<")[0] for e in tr]
    return {k: fam.count(k) for k in ("k_gemm_b9", "k_gemm_b9_h", "k_widen_f16")}, sorted({e for e in tr if e.startswith("k_gemm_b9")})


lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


prod = load_product()
kw = dict(SHAPES[args.shape])
if args.layers:
    kw["layers"] = args.layers
hp = make_hparams(**kw, ctx=PCTX)
m16 = prod.NewSyntheticModel(hp, 1234)
changed = m16.NarrowF16()
m32 = prod.NewSyntheticModel(hp, 1234)
legs = (("fp32", m32, False), ("f16 off", m16, False), ("f16 on", m16, True))
say(f"# tools/bench_f16_tiles.py --shape {args.shape} --layers {kw['layers']} --lengths {args.lengths} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {PCTX}; fp32 as generated, f16 = NarrowF16 of the same seed ({changed} of its matrix elements rounded)")
say("# legs alternate in ONE process; host clock around an Eval that ends in a synchronisation")
if args.note:
    say(f"# {args.note}")
for name, m, on in legs:
    counts, insts = tile_launches(m, on, LENGTHS[0])
    say(f"# {name:7s} at {LENGTHS[0]} tokens: {counts}  {' '.join(insts)}")
say()

verdicts = []
say("one Eval of n tokens at past 0, ms (best of 3 per leg)")
for n in LENGTHS:
    r = {name: [] for name in LEGS}
    for _ in range(args.repeats):
        for name, m, on in legs:
            r[name].append(prompt_leg(m, on, n))
    med = {name: sorted(r[name])[len(r[name]) // 2] for name in LEGS}
    ok = max(r["f16 on"]) < min(r["f16 off"])
    verdicts.append(ok)
    say(f"  {n:4d} tokens   " + "   ".join(f"{name} {'  '.join(f'{x:8.3f}' for x in r[name])}" for name in LEGS) +
        f"   on / off {med['f16 on'] / med['f16 off']:.3f}  on / fp32 {med['f16 on'] / med['fp32']:.3f}  "
        f"slowest on {max(r['f16 on']):.3f} vs fastest off {min(r['f16 off']):.3f}: {'faster' if ok else 'NOT faster'}")
say()
say(f"condition (slowest f16-on leg faster than the fastest f16-off leg at every measured length): {'holds' if all(verdicts) else 'DOES NOT HOLD'}")
say()
m32.free(); m16.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w" if args.fresh else "a") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
