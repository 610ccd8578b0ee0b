"""Q4_1 models on the weight-stream MFMA kernels (lh_ctx_set_q41_stream, DESIGN 3m "Native stream kernels"): the synthetic 7B quantised to Q4_1
(Model.QuantizeQ41) and its fp32 twin (the same blocks through Model.ExpandQ41), both resident, three legs alternating in ONE process so that drift of the
box hits all alike:

  fp32      the fp32 twin: k_stream_mm2 / k_stream_dma over its own matrices
  q41 off   the Q4_1 model with the switch off: every layer expanded into an fp32 image (k_expand_q41) in front of the same kernels
  q41 on    the Q4_1 model with the switch on: k_stream_mm2_q41 / k_stream_dma_q41 read the nibble and (d, m) planes

  ticks     lh_batch ticks of 9 / 16 / 32 / 48 pods, ms per tick (captured graph, host clock around a Decode that ends in a synchronisation)
  prompts   one Eval of 16 / 32 / 48 / 96 / 128 / 160 tokens at past 0, ms (best of 3 per leg and repeat)

No number is fixed in advance.  Per row count the table says whether the slowest q41-on leg beat the fastest q41-off leg IN THIS RUN and by how much the
medians differ, and how far q41-on stays from the fp32 twin.  Writes what it measured to profiles/q41_stream.txt (and prints it).
usage: python tools/bench_q41_stream.py [--shape 7B] [--layers 0] [--steps 24] [--repeats 3] [--pods 9,16,32,48] [--tokens 16,32,48,96,128,160] [--note TEXT]
                                        [--out profiles/q41_stream.txt]"""
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
ap.add_argument("--pods", default="9,16,32,48")
ap.add_argument("--tokens", default="16,32,48,96,128,160")
ap.add_argument("--note", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q41_stream.txt"))
args = ap.parse_args()

from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, load_product, make_hparams  # noqa: E402

CTX = 192
LEGS = ("fp32", "q41 off", "q41 on")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def tick_leg(m, on, pods, steps):
    b = Batch(m, CTX, pods)
    b.SetQ41Stream(on)
    prompts = [[(t + 7 * i) % m.hp.vocabSize for t in PROMPT] for i in range(pods)]
    first = b.Prompt(prompts)
    b.Decode(first, [len(PROMPT)] * pods, 3)                           # warm: eager tick + capture
    _, dt = timed(lambda: b.Decode(first, [len(PROMPT)] * pods, steps))
    assert b.batched
    b.free()
    return dt / steps * 1e3


def prompt_leg(m, on, n):
    c = m.NewContext(CTX, 1)
    c.SetQ41Stream(on)
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
hp = make_hparams(**kw, ctx=CTX)
mq = prod.NewSyntheticModel(hp, 1234).QuantizeQ41()
mf = prod.NewSyntheticModel(hp, 1234).QuantizeQ41()
mf.ExpandQ41()
assert mq.weight_type == 3 and mf.weight_type == 0
legs = (("fp32", mf, False), ("q41 off", mq, False), ("q41 on", mq, True))
say(f"# tools/bench_q41_stream.py --shape {args.shape} --layers {kw['layers']} --steps {args.steps} --repeats {args.repeats} --pods {args.pods} --tokens {args.tokens}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {CTX}; q41 = QuantizeQ41, fp32 = the same blocks through ExpandQ41 (identical values)")
say("# legs alternate in ONE process; host clock around calls that end in a synchronisation; ms, one figure per repeat")
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
        ok = max(r["q41 on"]) < min(r["q41 off"])
        verdicts.append((n, unit, ok))
        say(f"  {n:3d} {unit}   " + "   ".join(f"{name} {'  '.join(f'{x:7.3f}' for x in r[name])}" for name in LEGS) +
            f"   on / off {med['q41 on'] / med['q41 off']:.3f}  on / fp32 {med['q41 on'] / med['fp32']:.3f}  "
            f"slowest on {max(r['q41 on']):.3f} vs fastest off {min(r['q41 off']):.3f}: {'on beats off' if ok else 'on does NOT beat off'}")
    say()


table(f"lh_batch ticks, ms per tick over {args.steps} ticks", [int(x) for x in args.pods.split(",") if x], "pods", lambda m, on, n: tick_leg(m, on, n, args.steps))
table("one Eval of n tokens at past 0, ms (best of 3 per leg)", [int(x) for x in args.tokens.split(",") if x], "tokens", prompt_leg)
lost = [f"{n} {unit}" for n, unit, ok in verdicts if not ok]
say("q41 on beat q41 off (slowest on leg faster than the fastest off leg) at every measured row count" if not lost else
    "q41 on did NOT beat q41 off at: " + ", ".join(lost))
mq.free(); mf.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
