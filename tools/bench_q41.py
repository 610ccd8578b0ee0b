"""Q4_1 weights next to fp32 and block-int4 in one process: the synthetic model as it is (fp32), quantised to block-int4 (Model.QuantizeQ4)
and to Q4_1 (Model.QuantizeQ41), every measurement as alternating legs fp32 / Q4_0 / Q4_1 / fp32 / ... so that drift of the box hits all alike.  Host
clock around calls that end in a device synchronisation.  Appends what it measured to profiles/q41_decode.txt (and prints it); a figure that was not
measured is not written.  No speed is required of Q4_1: a loss to Q4_0 is recorded as it is.

  decode      the resident greedy loop (llamago_DecodeGreedyResident) and llamago_GreedyContinue (one lh_graph_compute per token), tok/s
  ticks       lh_batch ticks of 2 / 4 pods (one pass on the row kernels), ms per tick

fp32 7B needs 26 GB for its leg; --no-f32 leaves it out.
usage: python tools/bench_q41.py [--shape 7B] [--layers 0] [--steps 100] [--repeats 3] [--no-f32] [--out profiles/q41_decode.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-f32", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q41_decode.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, decode_greedy_resident, load_product, make_hparams  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def decode_leg(m, steps, contract):
    c = m.NewContext(128, 1)
    first = int(np.argmax(c.Eval(PROMPT, 0)))
    if contract:
        c.GreedyContinue(first, len(PROMPT), 4)                        # warm: the kept graph, the captured step
        _, dt = timed(lambda: c.GreedyContinue(first, len(PROMPT), steps))
    else:
        decode_greedy_resident(c, first, len(PROMPT), 8)
        _, dt = timed(lambda: decode_greedy_resident(c, first, len(PROMPT), steps))
    c.free()
    return steps / dt


def tick_leg(m, pods, steps):
    b = Batch(m, 128, pods)
    first = b.Prompt([[(t + 7 * i) % m.hp.vocabSize for t in PROMPT] for i in range(pods)])
    b.Decode(first, [len(PROMPT)] * pods, 3)                           # warm: eager tick + capture
    _, dt = timed(lambda: b.Decode(first, [len(PROMPT)] * pods, steps))
    b.free()
    return dt / steps * 1e3


prod = load_product()
kw = dict(SHAPES[args.shape])
if args.layers:
    kw["layers"] = args.layers
hp = make_hparams(**kw, ctx=128)
models = {} if args.no_f32 else {"fp32": prod.NewSyntheticModel(hp, 1234)}
models["Q4_0"] = prod.NewSyntheticModel(hp, 1234).QuantizeQ4()
models["Q4_1"] = prod.NewSyntheticModel(hp, 1234).QuantizeQ41()
lines = [f"## tools/bench_q41.py --shape {args.shape} --layers {kw['layers']} --steps {args.steps} --repeats {args.repeats}: alternating legs {' / '.join(models)}"]
rows = [("resident loop, tok/s", lambda m: decode_leg(m, args.steps, False)), ("contract route, tok/s", lambda m: decode_leg(m, args.steps, True)),
        ("tick of 2 pods, ms", lambda m: tick_leg(m, 2, args.steps)), ("tick of 4 pods, ms", lambda m: tick_leg(m, 4, args.steps))]
for what, leg in rows:
    got = {k: [] for k in models}
    for _ in range(args.repeats):
        for k, m in models.items():
            got[k].append(leg(m))
    lines.append(f"{what:24s} " + "   ".join(f"{k} " + " / ".join(f"{v:.2f}" for v in vs) for k, vs in got.items()))
for m in models.values():
    m.free()
print("\n".join(lines))
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
