"""lh_batch_feed against the routes it replaces, LLaMA-7B-shaped layers (results: profiles/feed_ragged.txt).  Wall time of the call on the host
(its synchronisation included), median of --reps after one warm-up call.
  a  time to the first tick for P pods with L-token prompts: one lh_batch_feed against lh_batch_prompt (one Eval per pod), fp32 and block-int8
  b  a 24-token prompt joins 32 pods that decode behind 1000 cached tokens: one feed (prompt rows + the 32 decode rows in one pass) against the prompt as an
     Eval of its own + a tick (the baseline's tick advances all 33 pods, the new one included, where the feed carries 32 decode rows: one row of 33 in
     the baseline's disfavour)
  c  one 64-token chunk behind 1984 cached tokens (ctx 2048): segment attention with QB = 2 / 4 / 8, the per-row kernels (LLAMAHIP_FEED_ROW_ATTN=1) and
     the pod's own Eval (LLAMAHIP_FEED_SOLO_MIN=1)
  d  one pod's n-token prompt, n = 65..256: batched passes against its solo Eval (sets FEED_SOLO_MIN)
  --sample  the sampled batch (lh_batch_feed_sample, the one-launch sampled tick; results: profiles/feed_sample.txt), instead of the parts above:
     sa  a sampled tick of 2 / 8 / 32 / 64 pods, topK 40: ONE sampler launch against LLAMAHIP_SAMPLE_PER_POD=1, same process and batch, alternating;
         per variant the median over --reps (>= 5) runs of --ticks ticks from the same positions, and the spread (max - min) between the runs
         (lh_batch_set rewinds the positions only: rings and draw counters go on, so the runs sample different states - the time does not depend on them)
     sb  a 24-token job joins 32 sampled pods: one lh_batch_feed_sample against what there was before it - sampler off, lh_batch_feed, sampler on again
         (which also empties every pod's ring and restarts its draw counter)
usage: python tools/bench_feed.py [a b c d] [--layers 32] [--layers-c 8] [--reps 3] [--int8]
       python tools/bench_feed.py --sample [--layers 32] [--reps 5] [--ticks 20]
BENCH_B_ONLY=feed|tick (environment): part b measures that variant only - one variant per process under a profiler"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from llama_go_amd.mlapi import SHAPES, Batch, load_product, make_hparams

ap = argparse.ArgumentParser()
ap.add_argument("parts", nargs="*", default=["a", "b", "c", "d"])
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--layers-c", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--int8", action="store_true", help="part a on block-int8 weights too")
ap.add_argument("--sample", action="store_true", help="the sampled-batch leg (sa, sb) instead of parts a-d")
ap.add_argument("--ticks", type=int, default=20, help="--sample: ticks per timed run")
args = ap.parse_args()
if args.sample:
    args.parts = ["sa", "sb"]
    args.reps = max(args.reps, 5)
prod = load_product()
rng = np.random.default_rng(0)


def med(fn, reps=args.reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(sorted(ts)[len(ts) // 2] * 1e3, 3)


def env(**kw):
    for k in ("LLAMAHIP_FEED_SOLO_MIN", "LLAMAHIP_FEED_QB", "LLAMAHIP_FEED_ROW_ATTN"):
        os.environ.pop(k, None)
    for k, v in kw.items():
        os.environ["LLAMAHIP_FEED_" + k] = str(v)


def model(layers, ctx, int8=False):
    kw = dict(SHAPES["7B"]); kw["layers"] = layers
    hp = make_hparams(**kw, ctx=ctx)
    m = prod.NewSyntheticModel(hp, 1234)
    if int8:
        m.QuantizeQ8()
    return m, hp


def toks(hp, n):
    return [int(t) for t in rng.integers(0, hp.vocabSize, n)]


if "a" in args.parts:
    for int8 in ([False, True] if args.int8 else [False]):
        m, hp = model(args.layers, 128, int8)
        for P, L in ((64, 2), (32, 4), (16, 8), (8, 16), (4, 64)):
            env()
            prompts = [toks(hp, L) for _ in range(P)]
            b = Batch(m, 128, P)
            feed = med(lambda: b.Feed(prompts, [0] * P))
            prompt = med(lambda: b.Prompt(prompts))
            same = b.Feed(prompts, [0] * P) == b.Prompt(prompts)
            b.free()
            print(json.dumps({"part": "a", "int8": int8, "layers": args.layers, "pods": P, "prompt_len": L, "feed_ms": feed, "batch_prompt_ms": prompt, "ratio": round(prompt / feed, 2), "same_ids": same}), flush=True)
        m.free()

if "b" in args.parts:
    ctx = 1100
    m, hp = model(args.layers, ctx)
    b = Batch(m, ctx, 33)
    env()
    ids = b.Feed([toks(hp, 1000) for _ in range(32)] + [toks(hp, 24)], [0] * 33)
    new = toks(hp, 24)
    state = {"ids": ids, "pos": [1000] * 32}

    def one_feed():
        env()
        out = b.Feed([[t] for t in state["ids"][:32]] + [new], state["pos"] + [0])
        state["ids"], state["pos"] = out, [p + 1 for p in state["pos"]]

    def eval_and_tick():
        env(SOLO_MIN=1)
        b.Feed([[]] * 32 + [new], [0] * 33)
        state["ids"], state["pos"] = b.Tick(), [p + 1 for p in state["pos"]]

    only = os.environ.get("BENCH_B_ONLY", "")   # (profiling: one variant per process)
    print(json.dumps({"part": "b", "layers": args.layers, "pods": 32, "cached": 1000, "prompt_len": 24, "one_feed_ms": med(one_feed) if only != "tick" else None,
                      "eval_plus_tick_ms": med(eval_and_tick) if only != "feed" else None}), flush=True)
    b.free()
    m.free()

if args.sample:
    from llama_go_amd.mlapi import FEED_NEW
    ctx, SMP = 256, dict(topK=40, topP=0.95, temp=0.8, repeatPenalty=1.1, seed=1)
    m, hp = model(args.layers, ctx)

    def switch(per_pod):
        if per_pod:
            os.environ["LLAMAHIP_SAMPLE_PER_POD"] = "1"
        else:
            os.environ.pop("LLAMAHIP_SAMPLE_PER_POD", None)

    for P in (2, 8, 32, 64):
        b = Batch(m, ctx, P)
        b.Feed([toks(hp, 8) for _ in range(P)], [0] * P)
        b.SetSampler(ringSize=ctx, **SMP)
        runs = {False: [], True: []}
        for rep in range(args.reps):
            for per_pod in (False, True):
                switch(per_pod)
                b.Set(None, [8] * P)          # every run from the same positions
                b.Tick(); b.Tick()            # the switch drops the captured tick: capture, one replay
                t0 = time.perf_counter()
                for _ in range(args.ticks):
                    b.Tick()
                runs[per_pod].append((time.perf_counter() - t0) / args.ticks * 1e3)
        switch(False)
        b.free()
        mid = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        spread = {k: max(v) - min(v) for k, v in runs.items()}
        print(json.dumps({"part": "sa", "layers": args.layers, "pods": P, "ticks_per_run": args.ticks, "runs": args.reps, "one_launch_tick_ms": round(mid[False], 4),
                          "per_pod_tick_ms": round(mid[True], 4), "one_launch_spread_ms": round(spread[False], 4), "per_pod_spread_ms": round(spread[True], 4),
                          "gain_us": round((mid[True] - mid[False]) * 1e3, 1),
                          "one_launch_slower_than_spread": bool(mid[False] - mid[True] > max(spread.values()))}), flush=True)

    b = Batch(m, ctx, 33)
    b.SetSampler(ringSize=ctx, **SMP)
    b.FeedSample([toks(hp, 64) for _ in range(32)] + [toks(hp, 24)], [0] * 33, [FEED_NEW] * 33)
    new = toks(hp, 24)

    def feed_sample():
        b.FeedSample([[]] * 32 + [new], [0] * 33, [0] * 32 + [FEED_NEW])

    def off_feed_on():
        b.ClearSampler()
        b.Feed([[]] * 32 + [new], [0] * 33)
        b.SetSampler(ringSize=ctx, **SMP)

    print(json.dumps({"part": "sb", "layers": args.layers, "pods": 32, "cached": 64, "prompt_len": 24, "runs": args.reps, "feed_sample_ms": med(feed_sample),
                      "sampler_off_feed_on_ms": med(off_feed_on)}), flush=True)
    b.free()
    m.free()

if "c" in args.parts:
    ctx, past, n = 2048, 1984, 64
    m, hp = model(args.layers_c, ctx)
    b = Batch(m, ctx, 2)
    seq = toks(hp, ctx)
    env()
    b.Feed([seq[:past], seq[:4]], [0, 0])
    res = {"part": "c", "layers": args.layers_c, "chunk": n, "past": past}
    for name, kw in (("seg_qb8_ms", dict(QB=8)), ("seg_qb4_ms", dict(QB=4)), ("seg_qb2_ms", dict(QB=2)), ("row_attn_ms", dict(ROW_ATTN=1)), ("solo_eval_ms", dict(SOLO_MIN=1))):
        env(**kw)
        res[name] = med(lambda: b.Feed([seq[past:], []], [past, 0]))
    print(json.dumps(res), flush=True)
    b.free()
    m.free()

if "d" in args.parts:
    m, hp = model(args.layers, 256)
    b = Batch(m, 256, 2)
    env()
    b.Feed([toks(hp, 2), toks(hp, 2)], [0, 0])
    for n in (65, 96, 128, 129, 160, 192, 224, 256):
        seq = toks(hp, n)
        env(SOLO_MIN=100000)
        batched = med(lambda: b.Feed([seq, []], [0, 0]))
        env(SOLO_MIN=1)
        solo = med(lambda: b.Feed([seq, []], [0, 0]))
        print(json.dumps({"part": "d", "layers": args.layers, "n": n, "batched_passes_ms": batched, "solo_eval_ms": solo}), flush=True)
    b.free()
    m.free()
env()
