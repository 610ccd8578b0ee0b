"""Block-int4 models on the bf16 stream kernel (lh_ctx_set_q4_stream, DESIGN 3l "Native stream kernel"): the synthetic 7B quantised to block-int4
(Model.QuantizeQ4) and its block-int8 twin (the same blocks through Model.ExpandQ4), both resident, three legs alternating in ONE process so that drift
of the box hits all alike:

  int8      the int8 twin: k_stream_q8b over its own int8 planes
  int4 off  the int4 model with the switch off: every layer expanded into an int8 image (k_expand_q4) in front of k_stream_q8b
  int4 on   the int4 model with the switch on: k_stream_q4b reads the nibbles

  ticks     lh_batch ticks of 5 / 8 / 16 / 32 / 48 / 64 pods, ms per tick (captured graph, host clock around a Decode that ends in a synchronisation)
  prompts   one Eval of 8 / 16 / 32 / 64 / 88 tokens at past 0, ms (best of 3 per leg and repeat)

No number is fixed in advance.  Per row count the table says whether the slowest int4-on leg beat the fastest int4-off leg IN THIS RUN and by how much the
medians differ, and how far int4-on stays from the int8 twin.  Writes what it measured to profiles/q4_stream.txt (and prints it).
usage: python tools/bench_q4_stream.py [--shape 7B] [--layers 0] [--steps 24] [--repeats 3] [--pods 5,8,16,32,48,64] [--tokens 8,16,32,64,88] [--note TEXT]
                                       [--out profiles/q4_stream.txt]"""
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
ap.add_argument("--pods", default="5,8,16,32,48,64")
ap.add_argument("--tokens", default="8,16,32,64,88")
ap.add_argument("--note", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q4_stream.txt"))
args = ap.parse_args()

from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, load_product, make_hparams  # noqa: E402

CTX = 128
LEGS = ("int8", "int4 off", "int4 on")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def tick_leg(m, on, pods, steps):
    b = Batch(m, CTX, pods)
    b.SetQ4Stream(on)
    prompts = [[(t + 7 * i) % m.hp.vocabSize for t in PROMPT] for i in range(pods)]
    first = b.Prompt(prompts)
    b.Decode(first, [len(PROMPT)] * pods, 3)                           # warm: eager tick + capture
    _, dt = timed(lambda: b.Decode(first, [len(PROMPT)] * pods, steps))
    assert b.batched
    b.free()
    return dt / steps * 1e3


def prompt_leg(m, on, n):
    c = m.NewContext(CTX, 1)
    c.SetQ4Stream(on)
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
m4 = prod.NewSyntheticModel(hp, 1234).QuantizeQ4()
m8 = prod.NewSyntheticModel(hp, 1234).QuantizeQ4()
m8.ExpandQ4()
assert m4.weight_type == 2 and m8.weight_type == 7
legs = (("int8", m8, False), ("int4 off", m4, False), ("int4 on", m4, True))
say(f"# tools/bench_q4_stream.py --shape {args.shape} --layers {kw['layers']} --steps {args.steps} --repeats {args.repeats} --pods {args.pods} --tokens {args.tokens}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {CTX}; int4 = QuantizeQ4, int8 = the same blocks through ExpandQ4 (identical values)")
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
        ok = max(r["int4 on"]) < min(r["int4 off"])
        verdicts.append((n, unit, ok))
        say(f"  {n:3d} {unit}   " + "   ".join(f"{name} {'  '.join(f'{x:7.3f}' for x in r[name])}" for name in LEGS) +
            f"   on / off {med['int4 on'] / med['int4 off']:.3f}  on / int8 {med['int4 on'] / med['int8']:.3f}  "
            f"slowest on {max(r['int4 on']):.3f} vs fastest off {min(r['int4 off']):.3f}: {'on beats off' if ok else 'on does NOT beat off'}")
    say()


table(f"lh_batch ticks, ms per tick over {args.steps} ticks", [int(x) for x in args.pods.split(",") if x], "pods", lambda m, on, n: tick_leg(m, on, n, args.steps))
table("one Eval of n tokens at past 0, ms (best of 3 per leg)", [int(x) for x in args.tokens.split(",") if x], "tokens", prompt_leg)
lost = [f"{n} {unit}" for n, unit, ok in verdicts if not ok]
say("int4 on beat int4 off (slowest on leg faster than the fastest off leg) at every measured row count" if not lost else
    "int4 on did NOT beat int4 off at: " + ", ".join(lost))
m4.free(); m8.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
