"""f16 weights kept f16 in HBM against the widened fp32 run of the same process: the synthetic 7B as fp32 and narrowed (Model.NarrowF16),
both resident, every measurement as alternating legs fp32 / f16 / fp32 / f16 ... so that drift of the box hits both alike.  Host clock around calls
that end in a device synchronisation.  Writes what it measured to profiles/f16_decode.txt (and prints it); a figure that was not measured is not written.

  decode      the resident greedy loop (llamago_DecodeGreedyResident) and llamago_GreedyContinue (one lh_graph_compute per token), tok/s
  ticks       lh_batch ticks of 2 / 4 / 8 pods (one f16 pass on k_gemv_rows_h) and of 16 pods (the widened route: its cost on record), ms per tick
  prompts     one Eval of 8 / 32 / 128 / 512 tokens, ms (8: k_gemv_rows_h; the others: the widened route)
  U sweep     LLAMAHIP_F16_U = 2 / 4 / 8 (rows in flight of the K = 4096 launches), each in a fresh child process (the switch is read once):
              per-kernel times of the wq|wk|wv and w1|w3 launches from lh_llama_profile_decode and the resident loop's tok/s

Condition (not a target): over the repeats, the slowest f16 one-stream decode leg is faster than the fastest fp32 leg.
usage: python tools/bench_f16.py [--shape 7B] [--layers 0] [--steps 100] [--repeats 3] [--no-sweep] [--out profiles/f16_decode.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIT_TOK_S = 406.0     # DESIGN 3a's per-launch fit (t = 3.2 us + bytes / 7.0 TB/s) over halved streams: a prediction, not a target

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_decode.txt"))
ap.add_argument("--child-u", type=int, default=0, help=argparse.SUPPRESS)
args = ap.parse_args()

import numpy as np  # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, decode_greedy_resident, load_product, make_hparams, profile_decode  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def model_pair(prod, kw, ctx, both=True):
    hp = make_hparams(**kw, ctx=ctx)
    m16 = prod.NewSyntheticModel(hp, 1234)
    changed = m16.NarrowF16()
    m32 = prod.NewSyntheticModel(hp, 1234) if both else None
    return hp, m32, m16, changed


def decode_leg(m, ctx_size, steps, contract):
    c = m.NewContext(ctx_size, 1)
    first = int(np.argmax(c.Eval(PROMPT, 0)))
    if contract:
        c.GreedyContinue(first, len(PROMPT), 4)                        # warm: the kept graph, the captured step
        ids, dt = timed(lambda: c.GreedyContinue(first, len(PROMPT), steps))
    else:
        decode_greedy_resident(c, first, len(PROMPT), 8)
        (ids, _), dt = timed(lambda: decode_greedy_resident(c, first, len(PROMPT), steps))
    c.free()
    return steps / dt, ids


def tick_leg(m, ctx_size, pods, steps):
    b = Batch(m, ctx_size, pods)
    prompts = [[(t + 7 * i) % m.hp.vocabSize for t in PROMPT] for i in range(pods)]
    first = b.Prompt(prompts)
    b.Decode(first, [len(PROMPT)] * pods, 3)                           # warm: eager tick + capture
    _, dt = timed(lambda: b.Decode(first, [len(PROMPT)] * pods, steps))
    batched = b.batched
    b.free()
    return dt / steps * 1e3, batched


def prompt_leg(m, ctx_size, n):
    c = m.NewContext(ctx_size, 1)
    toks = [(31 * i + 5) % m.hp.vocabSize for i in range(n)]
    c.Eval(toks, 0)                                                    # warm
    best = min(timed(lambda: c.Eval(toks, 0))[1] for _ in range(3))
    c.free()
    return best * 1e3


def child_u(u):
    """one U of the sweep, in this (fresh) process: LLAMAHIP_F16_U is already in the environment"""
    prod = load_product()
    kw = dict(SHAPES[args.shape])
    kw["layers"] = args.layers or 8                                    # per-kernel times do not depend on the depth
    hp, _, m16, _ = model_pair(prod, kw, 128, both=False)
    c = m16.NewContext(128, 1)
    first = int(np.argmax(c.Eval(PROMPT, 0)))
    decode_greedy_resident(c, first, len(PROMPT), 8)
    rates = [args.steps / timed(lambda: decode_greedy_resident(c, first, len(PROMPT), args.steps))[1] for _ in range(3)]
    kt = {k["name"]: round(k["avg_us"], 2) for k in profile_decode(c, first, len(PROMPT), 3)}
    c.free()
    m16.free()
    print("CHILD " + json.dumps({"u": u, "layers": kw["layers"], "tok_s": [round(r, 1) for r in rates], "kernels_us": kt}))


if args.child_u:
    child_u(args.child_u)
    sys.exit(0)

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


sweep = []
if not args.no_sweep:   # children first: the parent has not opened the GPU yet, and only one 7B model is resident at a time
    for u in (2, 4, 8):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-u", str(u), "--shape", args.shape, "--layers", str(args.layers), "--steps", str(args.steps)],
                           env=dict(os.environ, LLAMAHIP_F16_U=str(u)), capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode or not got:
            sys.exit(f"U sweep child for U = {u} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        sweep.append(json.loads(got[0][6:]))

prod = load_product()
kw = dict(SHAPES[args.shape])
if args.layers:
    kw["layers"] = args.layers
CTX, PCTX = 128, 640     # decode and ticks in the headline's window; the prompts need room for 512 tokens
hp, m32, m16, changed = model_pair(prod, kw, CTX)
legs = (("fp32", m32), ("f16", m16))
say(f"# tools/bench_f16.py --shape {args.shape} --layers {kw['layers']} --steps {args.steps} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {CTX} ({PCTX} for the prompts); fp32 as generated, f16 = NarrowF16 of the same seed ({changed} of its matrix elements rounded)")
say("# alternating legs in ONE process; host clock around calls that end in a synchronisation; spread = (max - min) / median over the repeats of a leg")
say()

res = {}
for what, contract in (("resident greedy loop", False), ("GreedyContinue (contract route)", True)):
    r = {name: [] for name, _ in legs}
    ids = {}
    for _ in range(args.repeats):
        for name, m in legs:
            rate, ids[name] = decode_leg(m, CTX, args.steps, contract)
            r[name].append(rate)
    res[what] = r
    say(f"{what}, tok/s over {args.steps} steps")
    for name, _ in legs:
        v = sorted(r[name])
        say(f"  {name:5s} {'  '.join(f'{x:7.1f}' for x in r[name])}   median {v[len(v) // 2]:7.1f}  spread {(v[-1] - v[0]) / v[len(v) // 2] * 100:4.1f} %")
    med = {name: sorted(r[name])[len(r[name]) // 2] for name, _ in legs}
    say(f"  f16 / fp32 = {med['f16'] / med['fp32']:.3f};  slowest f16 leg {min(r['f16']):.1f} vs fastest fp32 leg {max(r['fp32']):.1f}: "
        f"{'faster by more than the spread' if min(r['f16']) > max(r['fp32']) else 'NOT separated from the spread'}")
    if not contract:
        say(f"  fraction of the {FIT_TOK_S:.0f} tok/s DESIGN 3a's fit predicts for halved streams: {med['f16'] / FIT_TOK_S:.3f}" if args.shape == "7B" and not args.layers else
            "  (the 406 tok/s of DESIGN 3a's fit is for the full 7B: not compared)")
    say()

say("lh_batch ticks, ms per tick (2 / 4 / 8 pods: one pass on k_gemv_rows / k_gemv_rows_h; 16 pods: f16 on the widened route)")
for pods in (2, 4, 8, 16):
    r = {name: [] for name, _ in legs}
    for _ in range(args.repeats):
        for name, m in legs:
            ms, batched = tick_leg(m, CTX, pods, 24)
            r[name].append(ms)
    say(f"  {pods:2d} pods   fp32 {'  '.join(f'{x:7.3f}' for x in r['fp32'])}   f16 {'  '.join(f'{x:7.3f}' for x in r['f16'])}   f16 / fp32 (medians) "
        f"{sorted(r['f16'])[len(r['f16']) // 2] / sorted(r['fp32'])[len(r['fp32']) // 2]:.3f}")
say()

say("one Eval of n tokens at past 0, ms (best of 3 per leg; 8: the decode stream's rows; 32 / 128 / 512: f16 on the widened route = 2 B read + 4 B written + 4 B read per weight)")
for n in (8, 32, 128, 512):
    r = {name: [] for name, _ in legs}
    for _ in range(args.repeats):
        for name, m in legs:
            r[name].append(prompt_leg(m, PCTX, n))
    say(f"  n = {n:3d}   fp32 {'  '.join(f'{x:8.3f}' for x in r['fp32'])}   f16 {'  '.join(f'{x:8.3f}' for x in r['f16'])}   f16 / fp32 (medians) "
        f"{sorted(r['f16'])[len(r['f16']) // 2] / sorted(r['fp32'])[len(r['fp32']) // 2]:.3f}")
say()

if sweep:
    say(f"U sweep of the K = 4096 f16 launches (rows in flight per wave), {sweep[0]['layers']} layers, one fresh process per U; us per launch from lh_llama_profile_decode")
    for s in sweep:
        k = s["kernels_us"]
        say(f"  U = {s['u']}   wq|wk|wv {k.get('gemv_qkv_rope', float('nan')):7.2f} us   w1|w3 {k.get('gemv_w1w3_silu', float('nan')):7.2f} us   wo {k.get('gemv_wo_resid', float('nan')):6.2f} us   "
            f"w2 {k.get('gemv_w2_resid', float('nan')):6.2f} us   lm_head {k.get('gemv_lmhead', float('nan')):6.2f} us   resident loop {'  '.join(f'{x:7.1f}' for x in s['tok_s'])} tok/s")
    say()

c32, c16 = m32.NewContext(128, 1), m16.NewContext(128, 1)
first32, first16 = int(np.argmax(c32.Eval(PROMPT, 0))), int(np.argmax(c16.Eval(PROMPT, 0)))
say("per-kernel times of one decode step, us per launch (lh_llama_profile_decode): fp32 | f16")
k32 = {k["name"]: k for k in profile_decode(c32, first32, len(PROMPT), 3)}
k16 = {k["name"]: k for k in profile_decode(c16, first16, len(PROMPT), 3)}
for name in k32:
    if name in k16:
        say(f"  {name:18s} {k32[name]['avg_us']:8.2f} us {k32[name]['gbps']:8.0f} GB/s | {k16[name]['avg_us']:8.2f} us {k16[name]['gbps']:8.0f} GB/s")
c32.free(); c16.free(); m32.free(); m16.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
