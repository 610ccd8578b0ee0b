"""f16 models on the stream kernels of 2..128 rows (lh_ctx_set_f16_stream, DESIGN 3k "Native stream kernels"): the synthetic 7B as fp32 and narrowed
(Model.NarrowF16), both resident, three legs alternating in ONE process so that drift of the box hits all alike:

  fp32      the fp32 model
  f16 off   the f16 model with the switch off: every layer widened into an fp32 image in front of the fp32 stream kernels
  f16 on    the f16 model with the switch on: k_stream_mm2_h / k_stream_dma_h read the halves

  ticks     lh_batch ticks of 9 / 16 / 32 / 48 pods, ms per tick (captured graph, host clock around a Decode that ends in a synchronisation)
  prompts   one Eval of 16 / 32 / 48 / 96 / 128 / 160 tokens at past 0, ms (best of 3 per leg and repeat)

Condition the route ships under (not a target): at every measured row count the slowest f16-on leg is faster than the fastest f16-off leg.
Against fp32 the ratio of the medians is reported per row count.  Writes what it measured to profiles/f16_stream.txt (and prints it).
usage: python tools/bench_f16_stream.py [--shape 7B] [--layers 0] [--steps 24] [--repeats 3] [--note TEXT] [--out profiles/f16_stream.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--note", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_stream.txt"))
args = ap.parse_args()

from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, load_product, make_hparams  # noqa: E402

CTX, PCTX = 128, 192     # ticks in the headline's window; the prompts need room for 160 tokens
LEGS = ("fp32", "f16 off", "f16 on")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def tick_leg(m, on, pods, steps):
    b = Batch(m, CTX, pods)
    b.SetF16Stream(on)
    prompts = [[(t + 7 * i) % m.hp.vocabSize for t in PROMPT] for i in range(pods)]
    first = b.Prompt(prompts)
    b.Decode(first, [len(PROMPT)] * pods, 3)                           # warm: eager tick + capture
    _, dt = timed(lambda: b.Decode(first, [len(PROMPT)] * pods, steps))
    assert b.batched
    b.free()
    return dt / steps * 1e3


def prompt_leg(m, on, n):
    c = m.NewContext(PCTX, 1)
    c.SetF16Stream(on)
    toks = [(31 * i + 5) % m.hp.vocabSize for i in range(n)]
    c.Eval(toks, 0)                                                    # warm
    best = min(timed(lambda: c.Eval(toks, 0))[1] for _ in range(3))
    c.free()
    return best * 1e3


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
say(f"# tools/bench_f16_stream.py --shape {args.shape} --layers {kw['layers']} --steps {args.steps} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {CTX} for the ticks and {PCTX} for the prompts; fp32 as generated, f16 = NarrowF16 of the same seed "
    f"({changed} of its matrix elements rounded)")
say("# legs alternate in ONE process; host clock around calls that end in a synchronisation")
if args.note:
    say(f"# {args.note}")
say()

verdicts = []


def table(title, counts, unit, leg_fn):
    say(title)
    for n in counts:
        r = {name: [] for name in LEGS}
        for _ in range(args.repeats):
            for name, m, on in legs:
                r[name].append(leg_fn(m, on, n))
        med = {name: sorted(r[name])[len(r[name]) // 2] for name in LEGS}
        ok = max(r["f16 on"]) < min(r["f16 off"])
        verdicts.append(ok)
        say(f"  {n:3d} {unit}   " + "   ".join(f"{name} {'  '.join(f'{x:7.3f}' for x in r[name])}" for name in LEGS) +
            f"   on / off {med['f16 on'] / med['f16 off']:.3f}  on / fp32 {med['f16 on'] / med['fp32']:.3f}  "
            f"slowest on {max(r['f16 on']):.3f} vs fastest off {min(r['f16 off']):.3f}: {'faster' if ok else 'NOT faster'}")
    say()


table(f"lh_batch ticks, ms per tick over {args.steps} ticks", (9, 16, 32, 48), "pods", lambda m, on, n: tick_leg(m, on, n, args.steps))
table("one Eval of n tokens at past 0, ms (best of 3 per leg)", (16, 32, 48, 96, 128, 160), "tokens", prompt_leg)
say(f"condition (slowest f16-on leg faster than the fastest f16-off leg at every measured row count): {'holds' if all(verdicts) else 'DOES NOT HOLD'}")
m32.free(); m16.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
