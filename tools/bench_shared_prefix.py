"""Ticks of pods that share a prompt prefix (lh_batch_fork; results: profiles/shared_prefix.txt): ms per captured tick with the shared tick
kernel (k_attention_split_shared, QB = 4 and QB = 8) against the per-row kernels (LLAMAHIP_SHARE_ROW_ATTN=1: the launch sequence of a batch that never
forked), synthetic LLaMA-7B layers, ctx 2048, fp32 and block-int8.
  - P pods (8 / 16 / 32 / 64) in ONE group behind T shared keys (256 / 1024 / 1920): pod 0 evaluates a T-token prompt, lh_batch_fork hands it to the others,
    lh_batch_set places every pod at T;
  - one mixed case: two groups (8 pods behind 1024 keys, 8 behind 512) and four loners behind 300 keys of their own.
All variants run in the SAME process on the same batch, alternating, after warm-up: per repetition and variant the pods are put back at their positions,
two untimed ticks re-capture the tick for the variant, then --ticks ticks are timed (host wall time of lh_batch_decode: one graph launch per tick, one
wait at the end).  Per variant: the median over --reps and the spread (max - min).  The ids of all variants must be equal.
  - --group-size G: the P pods as P / G groups of G members, every group behind T keys of its own (sets LLAMAHIP_SHARE_MIN).
usage: python tools/bench_shared_prefix.py [--layers 32] [--reps 5] [--ticks 16] [--pods 8,16,32,64] [--keys 256,1024,1920] [--group-size 0] [--int8-too | --int8-only] [--no-mixed]
       python tools/bench_shared_prefix.py --profile shared4|shared8|row --pods 32 --keys 1024     (one variant only: a kernel-trace run of its own)"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from llama_go_amd.mlapi import SHAPES, Batch, load_product, make_hparams

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ticks", type=int, default=16)
ap.add_argument("--pods", default="8,16,32,64")
ap.add_argument("--keys", default="256,1024,1920")
ap.add_argument("--group-size", type=int, default=0, help="cut the P pods into groups of this size, each behind a prefix of its own (0: one group)")
ap.add_argument("--int8-too", action="store_true")
ap.add_argument("--int8-only", action="store_true")
ap.add_argument("--no-mixed", action="store_true")
ap.add_argument("--profile", default="", help="run this variant alone (shared4, shared8, row), no alternation: for a profiler")
args = ap.parse_args()
CTX = 2048
VARIANTS = {"shared4": dict(LLAMAHIP_SHARE_ROW_ATTN="0", LLAMAHIP_SHARE_QB="4"), "shared8": dict(LLAMAHIP_SHARE_ROW_ATTN="0", LLAMAHIP_SHARE_QB="8"),
            "row": dict(LLAMAHIP_SHARE_ROW_ATTN="1", LLAMAHIP_SHARE_QB="4")}
prod = load_product()
rng = np.random.default_rng(0)


def place(m, hp, groups, loners):
    """groups: [(pods, keys)], loners: [keys] -> a batch whose groups share their prefixes, every pod standing behind its keys"""
    P = sum(n for n, _ in groups) + len(loners)
    b = Batch(m, CTX, P)
    feed, pos, forks, p = [], [], [], 0
    for n, keys in groups:
        feed += [[int(t) for t in rng.integers(0, hp.vocabSize, keys)]] + [[1]] * (n - 1)
        forks.append((p, list(range(p + 1, p + n)), keys))
        pos += [keys] * n
        p += n
    for keys in loners:
        feed.append([int(t) for t in rng.integers(0, hp.vocabSize, keys)])
        pos.append(keys)
    b.Feed(feed, [0] * P)
    for src, dst, keys in forks:
        if dst:
            b.Fork(src, dst, keys)
    return b, pos


def measure(b, pos, names):
    P = len(pos)
    toks = [int(t) for t in rng.integers(0, 32000, P)]
    times, ids = {k: [] for k in names}, {}
    for rep in range(args.reps + 1):          # (repetition 0 is the warm-up)
        for k in names:
            os.environ.update(VARIANTS[k])
            b.Decode(toks, pos, 2)            # the tick is captured anew for this variant
            t0 = time.perf_counter()
            got = b.Decode(toks, pos, args.ticks)
            dt = time.perf_counter() - t0
            if rep:
                times[k].append(dt / args.ticks * 1e3)
            ids[k] = got
    out = {"ids_equal": all(ids[k] == ids[names[0]] for k in names)}
    for k in names:
        ts = sorted(times[k])
        out[k + "_ms"] = round(ts[len(ts) // 2], 4)
        out[k + "_spread_ms"] = round(ts[-1] - ts[0], 4)
    return out


names = [args.profile] if args.profile else ["shared4", "shared8", "row"]
for int8 in ([True] if args.int8_only else [False, True] if args.int8_too else [False]):
    kw = dict(SHAPES["7B"]); kw["layers"] = args.layers
    hp = make_hparams(**kw, ctx=CTX)
    m = prod.NewSyntheticModel(hp, 1234)
    if int8:
        m.QuantizeQ8()
    for P in [int(x) for x in args.pods.split(",")]:
        for T in [int(x) for x in args.keys.split(",")]:
            G = args.group_size or P
            b, pos = place(m, hp, [(G, T)] * (P // G), [])
            r = measure(b, pos, names)
            b.free()
            print(json.dumps(dict({"case": "one group" if G == P else f"groups of {G}", "int8": int8, "layers": args.layers, "pods": P, "shared_keys": T, "ticks": args.ticks, "reps": args.reps}, **r)), flush=True)
    if not args.no_mixed and not args.profile:
        b, pos = place(m, hp, [(8, 1024), (8, 512)], [300] * 4)
        r = measure(b, pos, names)
        b.free()
        print(json.dumps(dict({"case": "mixed: 8 pods behind 1024 shared keys, 8 behind 512, 4 loners behind 300", "int8": int8, "layers": args.layers, "pods": 20,
                               "ticks": args.ticks, "reps": args.reps}, **r)), flush=True)
    m.free()
