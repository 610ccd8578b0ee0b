"""fp32 prompts of 65..128 tokens in ONE pass on k_stream_b9w (lh_ctx_set_wide_planes): the synthetic 7B, one Eval of n tokens at past 0, two
legs alternating in ONE process so that drift of the box hits both alike:

  off   the switch off: k_stream_dma, fp32-input MFMAs (what every context runs by default)
  on    the switch on: k_stream_b9w, eight exact bf16 products per weight over activation planes

A measurement is the mean over --evals back-to-back Evals (host clock around calls that end in a synchronisation; every Eval of a prompt reads its
logits back), taken --repeats times per leg and length, the legs alternating; both contexts are warmed with every length first.  Recorded per length:
every measurement, the medians' ratio, and whether the SLOWEST on leg beats the FASTEST off leg.  Beside them the two floors of DESIGN 3b (not
measured here): the weight stream of a 7B Eval, about 3.3 ms, and the exact-split bf16 roof, about 5.4 ms.  Per-launch times and the shader clock are
not collected.  Writes what it measured to profiles/wide_planes.txt (and prints it).
usage: python tools/bench_wide_planes.py [--shape 7B] [--layers 0] [--evals 20] [--repeats 5] [--note TEXT] [--out profiles/wide_planes.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_planes.txt"))
args = ap.parse_args()

from llama_go_amd.mlapi import SHAPES, load_product, make_hparams, route_trace  # noqa: E402

CTX = 128
LENGTHS = (65, 80, 96, 112, 128)
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
m = prod.NewSyntheticModel(hp, 1234)
ctxs = {"off": m.NewContext(CTX, 1), "on": m.NewContext(CTX, 1)}
ctxs["on"].SetWidePlanes(True)
toks = {n: [(31 * i + 5) % hp.vocabSize for i in range(n)] for n in LENGTHS}
for name, c in ctxs.items():           # warm every length on both legs; the legs must be on the kernels they are named for
    for n in LENGTHS:
        _, tr = route_trace(lambda: c.Eval(toks[n], 0))
        assert any(e.startswith("k_stream_b9w<") for e in tr) == (name == "on") and any(e.startswith("k_stream_dma<") for e in tr) == (name == "off"), (name, n, tr)

say(f"# tools/bench_wide_planes.py --shape {args.shape} --layers {kw['layers']} --evals {args.evals} --repeats {args.repeats}")
say(f"# synthetic {args.shape} seed 1234, fp32, {kw['layers']} layers, context {CTX}; one Eval of n tokens at past 0, ms per Eval (mean of {args.evals} back to back)")
say("# legs alternate in ONE process; host clock around calls that end in a synchronisation; both legs warmed with every length first")
say("# floors (DESIGN 3b, not measured here): weight stream about 3.3 ms per Eval, exact-split bf16 roof about 5.4 ms")
say("# per-launch times: not measured.  shader clock: not measured.")
if args.note:
    say(f"# {args.note}")
say()
wins = []
for n in LENGTHS:
    r = {"off": [], "on": []}
    for _ in range(args.repeats):
        for name in ("off", "on"):
            r[name].append(measure(ctxs[name], toks[n]))
    med = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
    ok = max(r["on"]) < min(r["off"])
    wins.append((n, ok))
    say(f"  {n:3d} tokens   " + "   ".join(f"{k} {'  '.join(f'{x:7.3f}' for x in r[k])}" for k in ("off", "on")) +
        f"   on / off {med['on'] / med['off']:.3f}   slowest on {max(r['on']):.3f} vs fastest off {min(r['off']):.3f}: {'faster' if ok else 'NOT faster'}")
say()
say("slowest on leg beats the fastest off leg at: " + (", ".join(str(n) for n, ok in wins if ok) or "no length") +
    "; not at: " + (", ".join(str(n) for n, ok in wins if not ok) or "no length"))
for c in ctxs.values():
    c.free()
m.free()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
