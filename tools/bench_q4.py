"""Block-int4 weights against block-int8 in one process: the synthetic 7B quantised to block-int8 (Model.QuantizeQ8) and to block-int4
(Model.QuantizeQ4), both resident, every measurement as alternating legs int8 / int4 / int8 / int4 ... so that drift of the box hits both alike.  Host
clock around calls that end in a device synchronisation.  Writes what it measured to profiles/q4_decode.txt (and prints it); a figure that was not
measured is not written.

  decode      the resident greedy loop (llamago_DecodeGreedyResident) and llamago_GreedyContinue (one lh_graph_compute per token), tok/s
  ticks       lh_batch ticks of 2 / 4 pods (one pass on k_gemv_q4_rows) and of 8 / 16 pods (the expanded route: its cost on record), ms per tick
  prompts     one Eval of 32 / 128 / 512 tokens, ms (the expanded route: 0.5 B read + 1 B written + 1 B read per weight)
  U sweep     LLAMAHIP_Q4_U = 2 / 4 / 8 and the shipped choice (rows in flight of the K = 4096 launches), each in a fresh child process (the switch is
              read once): per-kernel times from lh_llama_profile_decode and the resident loop's tok/s

Condition (not a target): over the repeats, the slowest int4 one-stream decode leg is faster than the fastest int8 leg.
usage: python tools/bench_q4.py [--shape 7B] [--layers 0] [--steps 100] [--repeats 3] [--no-sweep] [--out profiles/q4_decode.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIT_TOK_S = 900.0     # DESIGN 3a's per-launch fit (t = 3.2 us + bytes / 7.0 TB/s) over 20/36 of the int8 streams: a ceiling, not a target

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="7B")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q4_decode.txt"))
ap.add_argument("--child-u", type=int, default=-1, help=argparse.SUPPRESS)
args = ap.parse_args()

import numpy as np  # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, Batch, decode_greedy_resident, load_product, make_hparams, profile_decode  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def model_pair(prod, kw, ctx, both=True):
    hp = make_hparams(**kw, ctx=ctx)
    m4 = prod.NewSyntheticModel(hp, 1234).QuantizeQ4()
    m8 = prod.NewSyntheticModel(hp, 1234).QuantizeQ8() if both else None
    return hp, m8, m4


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
    """one U of the sweep, in this (fresh) process: LLAMAHIP_Q4_U is already in the environment (u = 0: unset, the shipped choice)"""
    prod = load_product()
    kw = dict(SHAPES[args.shape])
    kw["layers"] = args.layers or 8                                    # per-kernel times do not depend on the depth
    hp, _, m4 = model_pair(prod, kw, 128, both=False)
    c = m4.NewContext(128, 1)
    first = int(np.argmax(c.Eval(PROMPT, 0)))
    decode_greedy_resident(c, first, len(PROMPT), 8)
    rates = [args.steps / timed(lambda: decode_greedy_resident(c, first, len(PROMPT), args.steps))[1] for _ in range(3)]
    kt = {k["name"]: round(k["avg_us"], 2) for k in profile_decode(c, first, len(PROMPT), 3)}
    c.free()
    m4.free()
    print("CHILD " + json.dumps({"u": u, "layers": kw["layers"], "tok_s": [round(r, 1) for r in rates], "kernels_us": kt}))


if args.child_u >= 0:
    child_u(args.child_u)
    sys.exit(0)

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


sweep = []
if not args.no_sweep:   # children first: the parent has not opened the GPU yet, and only one 7B model is resident at a time
    for u in (2, 4, 8, 0):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-u", str(u), "--shape", args.shape, "--layers", str(args.layers), "--steps", str(args.steps)],
                           env=dict(os.environ, LLAMAHIP_Q4_U=str(u)), capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode or not got:
            sys.exit(f"U sweep child for U = {u} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        sweep.append(json.loads(got[0][6:]))

prod = load_product()
kw = dict(SHAPES[args.shape])
if args.layers:
    kw["layers"] = args.layers
CTX, PCTX = 128, 640     # decode and ticks in the headline's window; the prompts need room for 512 tokens
hp, m8, m4 = model_pair(prod, kw, CTX)
legs = (("int8", m8), ("int4", m4))
say(f"# tools/bench_q4.py --shape {args.shape} --layers {kw['layers']} --steps {args.steps} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, {kw['layers']} layers, context {CTX} ({PCTX} for the prompts); int8 = QuantizeQ8 and int4 = QuantizeQ4 of the same seed")
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
    say(f"  int4 / int8 = {med['int4'] / med['int8']:.3f};  slowest int4 leg {min(r['int4']):.1f} vs fastest int8 leg {max(r['int8']):.1f}: "
        f"{'faster by more than the spread' if min(r['int4']) > max(r['int8']) else 'slower by more than the spread' if max(r['int4']) < min(r['int8']) else 'NOT separated from the spread'}")
    if not contract:
        say(f"  fraction of the {FIT_TOK_S:.0f} tok/s ceiling DESIGN 3a's fit gives for 20/36 of the int8 bytes: {med['int4'] / FIT_TOK_S:.3f}" if args.shape == "7B" and not args.layers else
            "  (the 900 tok/s of DESIGN 3a's fit is for the full 7B: not compared)")
    say()

say("lh_batch ticks, ms per tick (2 / 4 pods: one pass on k_gemv_q8_rows / k_gemv_q4_rows; 8 / 16 pods: int8 on k_stream_q8b, int4 the same behind the expansion)")
for pods in (2, 4, 8, 16):
    r = {name: [] for name, _ in legs}
    for _ in range(args.repeats):
        for name, m in legs:
            ms, batched = tick_leg(m, CTX, pods, 24)
            r[name].append(ms)
    say(f"  {pods:2d} pods   int8 {'  '.join(f'{x:7.3f}' for x in r['int8'])}   int4 {'  '.join(f'{x:7.3f}' for x in r['int4'])}   int4 / int8 (medians) "
        f"{sorted(r['int4'])[len(r['int4']) // 2] / sorted(r['int8'])[len(r['int8']) // 2]:.3f}")
say()

say("one Eval of n tokens at past 0, ms (best of 3 per leg; int4 on the expanded route = 0.5 B read + 1 B written + 1 B read per weight)")
for n in (32, 128, 512):
    r = {name: [] for name, _ in legs}
    for _ in range(args.repeats):
        for name, m in legs:
            r[name].append(prompt_leg(m, PCTX, n))
    say(f"  n = {n:3d}   int8 {'  '.join(f'{x:8.3f}' for x in r['int8'])}   int4 {'  '.join(f'{x:8.3f}' for x in r['int4'])}   int4 / int8 (medians) "
        f"{sorted(r['int4'])[len(r['int4']) // 2] / sorted(r['int8'])[len(r['int8']) // 2]:.3f}")
say()

if sweep:
    say(f"U sweep of the K = 4096 int4 launches (rows in flight per register set; U = 0: the switch unset = the shipped choice, 4), {sweep[0]['layers']} layers, one fresh process per U; us per launch from lh_llama_profile_decode")
    for s in sweep:
        k = s["kernels_us"]
        say(f"  U = {s['u']}   wq|wk|wv {k.get('gemv_qkv_rope', float('nan')):7.2f} us   w1|w3 {k.get('gemv_w1w3_silu', float('nan')):7.2f} us   wo {k.get('gemv_wo_resid', float('nan')):6.2f} us   "
            f"w2 {k.get('gemv_w2_resid', float('nan')):6.2f} us   lm_head {k.get('gemv_lmhead', float('nan')):6.2f} us   resident loop {'  '.join(f'{x:7.1f}' for x in s['tok_s'])} tok/s")
    say()

c8, c4 = m8.NewContext(128, 1), m4.NewContext(128, 1)
first8, first4 = int(np.argmax(c8.Eval(PROMPT, 0))), int(np.argmax(c4.Eval(PROMPT, 0)))
say("per-kernel times of one decode step, us per launch (lh_llama_profile_decode): int8 | int4")
k8 = {k["name"]: k for k in profile_decode(c8, first8, len(PROMPT), 3)}
k4 = {k["name"]: k for k in profile_decode(c4, first4, len(PROMPT), 3)}
for name in k8:
    if name in k4:
        say(f"  {name:18s} {k8[name]['avg_us']:8.2f} us {k8[name]['gbps']:8.0f} GB/s | {k4[name]['avg_us']:8.2f} us {k4[name]['gbps']:8.0f} GB/s")
c8.free(); c4.free(); m8.free(); m4.free()

r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), "--filter", "q4"], capture_output=True, text=True)
isa = [ln for ln in r.stdout.splitlines() if " scratch " in ln and "kernels," not in ln]
if isa:
    spill = [ln for ln in isa if not ln.rstrip().endswith("scratch     0 vgpr_spill   0 sgpr_spill   0")]
    say()
    say(f"tools/isa_check.py --filter q4: {len(isa)} kernels (k_gemv_q4s / k_gemv_q4_rows instantiations, k_expand_q4, k_quantize_q4, k_q4_deinterleave), "
        f"{len(spill)} with scratch or spills")
    for ln in isa:
        say("  " + " ".join(ln.split()))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
