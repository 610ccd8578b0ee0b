"""Lookup-draft speculative decoding against the routes it rides on, LLaMA-7B shape (results: profiles/speculative.txt).
Host wall time of the calls (their synchronisations included), median of --reps after a warm-up call.  The weights are synthetic: acceptance
rates here are those of a replayed or a random text, never a model result.
  pass    cost of a verify pass of R rows (fp32 2 / 4 / 8, block-int8 2 / 4) behind 100 and behind 1000 cached tokens: the loop's own wall time /
          passes on a replay workload (corpus = the greedy run itself, so every pass is full), against a tick of R pods of lh_batch_decode at the
          same positions in the same process (existing code), and against the one-token resident step
  golden  the 7B golden workload (8-token prompt, ctx 128, 99 ids): the loop with the replay corpus (acceptance 1: the ceiling), without a corpus
          (the honest side), and lh_llama_decode_greedy, tokens/s each; the break-even mean of accepted ids per pass from the measured times
  --sample  the sampled route instead (lh_llama_decode_sample_lookup; results: profiles/sample_lookup.txt): the golden prompt, ctx 128, 100 sampled ids
          (topK 40, topP 0.95, temp 0.8, penalty 1.1): an R-row sampled pass against one plain sampled step of SampleDecode (prompt Eval and first
          sample taken off both by a 1-id call), the loop with the replay corpus (the ceiling) and without one, the break-even acceptance
  --pods P  the pods of a batch instead (lh_batch_decode_lookup; results: profiles/batch_lookup.txt): P pods behind the golden prompt, ctx 256, 96 ids
          per pod, draft_max 1 / 3 / 7 (R lowered to what P pods leave room for): a pass of P * R rows against a tick of P rows of lh_batch_decode, same
          process, alternating; aggregate tokens/s with the replay corpus (acceptance 1 by construction: a CEILING, not a model result), without a
          corpus, and of the plain ticks; the break-even mean of accepted ids per pod and pass
  --pods P --sample  the pods of a SAMPLING batch (lh_batch_decode_sample_lookup; results: profiles/batch_sample_lookup.txt): the same P pods, ctx 256, 96
          sampled ids per pod (topK 40, topP 0.95, temp 0.8, penalty 1.1), draft_max 1 / 3 / 7, every start a SetSampler + FeedSample(NEW + prompt) that is
          timed on its own and taken off: a sampled pass of P * R rows against a plain sampled tick of P pods of lh_batch_decode, same process,
          alternating; the sampler launch over P * R rows (lh_sample_pod_rows) against the tick's launch over P rows (lh_sample_pods), both as host twins
          whose wall time INCLUDES the upload of their logits; the loop with the replay corpus (the corpus is the run itself: acceptance 1 by
          construction, a CEILING, never a model result) and with no corpus; the break-even mean of accepted ids per pod and pass.
          The KERNEL time of the sampler launches is not a host figure: run this part under a kernel trace, one row count per run, the layer count being
          of no matter to the sampler -
            rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_speculative.py --pods P --sample --draft-max K --layers 2 --reps 2
          - and read k_sample_small_pod_rows (P * R workgroups, the passes) against k_sample_small_pods (P workgroups, the ticks) in the kernel statistics
usage: python tools/bench_speculative.py [pass golden] [--sample] [--pods P] [--draft-max K] [--layers 32] [--reps 5] [--int8] [--out profiles/speculative.txt]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from llama_go_amd.mlapi import FEED_NEW, PROMPT, SHAPES, Batch, SamplePods, decode_greedy_resident, load_product, make_hparams, sample_pod_rows

ap = argparse.ArgumentParser()
ap.add_argument("parts", nargs="*", default=["pass", "golden"])
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--int8", action="store_true", help="block-int8 weights too")
ap.add_argument("--sample", action="store_true", help="the sampled route (SampleDecodeLookup against SampleDecode) instead of the greedy parts")
ap.add_argument("--pods", type=int, default=0, help="the pods of a batch (Batch.DecodeLookup against the ticks of lh_batch_decode) instead of the solo parts")
ap.add_argument("--draft-max", type=int, default=0, help="--pods P --sample: this draft_max only (default: 1, 3 and 7)")
ap.add_argument("--out", default=None, help="append the result lines to this file")
args = ap.parse_args()
prod = load_product()
lines = []


def emit(d):
    s = json.dumps(d)
    print(s, flush=True)
    lines.append(s)


def med(fn, reps=args.reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3


def model(ctx, int8):
    kw = dict(SHAPES["7B"]); kw["layers"] = args.layers
    m = prod.NewSyntheticModel(make_hparams(**kw, ctx=ctx), 1234)
    if int8:
        m.QuantizeQ8()
    return m


def prompt_state(m, ctx, prompt):
    c = m.NewContext(ctx, 1)
    return c, int(np.argmax(c.Eval(prompt, 0)))


if args.sample and args.pods:
    args.parts = []
    P, ctx, n = args.pods, 256, 96
    SMP = dict(topK=40, topP=0.95, temp=0.8, repeatPenalty=1.1, seed=1234)
    prompts = [[PROMPT[0]] + [(t + 17 * i) % 32000 for t in PROMPT[1:]] for i in range(P)]
    past = [len(p) for p in prompts]
    for int8 in ([False, True] if args.int8 else [False]):
        m = model(ctx, int8)
        b = Batch(m, ctx, P)

        def head():   # what every leg starts with: a new job on every pod, its first id pending
            b.SetSampler(ringSize=ctx, **SMP)
            return b.FeedSample(prompts, [0] * P, [FEED_NEW] * P)
        first = head()
        run = b.Decode(first, past, n)
        replay = [t for p, f, gi in zip(prompts, first, run) for t in list(p) + [f] + gi]
        for K in ((args.draft_max,) if args.draft_max else (1, 3, 7)):
            res = {}

            def loop(corpus):
                ids, _, st, _ = b.DecodeSampleLookup(head(), past, n, K, 3, 1, corpus)
                res.update(rows=st[0]["rows"], passes=max(s["passes"] for s in st), accepted=sum(s["accepted"] for s in st), pod_passes=sum(s["passes"] for s in st),
                           same_ids=ids == run)

            def ticks():
                b.Decode(head(), past, n)
            ts = {"head": [], "replay": [], "ticks": [], "no_corpus": []}
            legs = (("head", head), ("replay", lambda: loop(replay)), ("ticks", ticks), ("no_corpus", lambda: loop(None)))
            for _, fn in legs:
                fn()
            shape = {}
            for _ in range(args.reps):
                for name, fn in legs:
                    t0 = time.perf_counter(); fn(); ts[name].append((time.perf_counter() - t0) * 1e3)
                    if name in ("replay", "no_corpus"):
                        shape[name] = dict(res)
            md = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            R = shape["replay"]["rows"]
            if R == 1:
                emit(dict(part="pods_sample", int8=int8, layers=args.layers, pods=P, draft_max=K, rows=1, note="no room for a second row: plain sampled ticks"))
                continue
            tick_ms = (md["ticks"] - md["head"]) / n
            out = dict(part="pods_sample", int8=int8, layers=args.layers, pods=P, draft_max=K, rows=R, pass_rows=P * R, ids_per_pod=n, head_ms=round(md["head"], 3),
                       tick_ms=round(tick_ms, 3), ticks_tok_s=round(P * n / (md["ticks"] - md["head"]) * 1e3, 1))
            for name in ("replay", "no_corpus"):
                ms = md[name] - md["head"]
                out.update({f"{name}_passes": shape[name]["passes"], f"{name}_accepted_per_pod_pass": round(shape[name]["accepted"] / shape[name]["pod_passes"], 3),
                            f"{name}_pass_ms": round(ms / shape[name]["passes"], 3), f"{name}_tok_s": round(P * n / ms * 1e3, 1),
                            f"{name}_ids_equal_ticks": shape[name]["same_ids"]})
            out["replay_is"] = "acceptance-1 ceiling (the corpus is the run itself), not a model result"
            out["pass_over_tick"] = round(out["no_corpus_pass_ms"] / tick_ms, 3)
            # the route wins when ids per pod and pass = 1 + mean accepted > pass time / tick time
            out["break_even_accepted_per_pod_pass"] = round(out["no_corpus_pass_ms"] / tick_ms - 1, 3)
            # the sampler launches alone, as host twins on random logits (their wall time includes the upload of P * R resp. P rows of 32000 floats)
            rng = np.random.default_rng(K)
            lg = (rng.standard_normal((P * R, 32000)) * 4).astype(np.float32)
            rings, rpos, draws = np.zeros((P, ctx), np.uint32), [0] * P, list(range(P))
            toks = rng.integers(0, 32000, (P, R)).astype(np.uint32)
            lg_ticks = np.ascontiguousarray(lg[::R])
            tw = {"pod_rows": [], "pods": []}
            twins = (("pod_rows", lambda: sample_pod_rows(prod, lg, rings, rpos, draws, toks, [R - 1] * P, **SMP)),
                     ("pods", lambda: SamplePods(prod, lg_ticks, rings, rpos, draws, **SMP)))
            for _, fn in twins:
                fn()
            for _ in range(args.reps):
                for name, fn in twins:
                    t0 = time.perf_counter(); fn(); tw[name].append((time.perf_counter() - t0) * 1e3)
            out["sampler_twin_pod_rows_ms"] = round(sorted(tw["pod_rows"])[len(tw["pod_rows"]) // 2], 3)
            out["sampler_twin_pods_ms"] = round(sorted(tw["pods"])[len(tw["pods"]) // 2], 3)
            out["sampler_twins_include"] = "the upload of their logits rows"
            emit(out)
        b.free()
        m.free()
    args.sample, args.pods = False, 0

if args.sample:
    args.parts = []
    SMP = dict(topK=40, topP=0.95, temp=0.8, repeatPenalty=1.1, seed=1234)
    for int8 in ([False, True] if args.int8 else [False]):
        K, n = 3 if int8 else 7, 100
        m = model(128, int8)
        c = m.NewContext(128, 1)
        run = c.SampleDecode(PROMPT, n, **SMP)
        head_ms = med(lambda: c.SampleDecode(PROMPT, 1, **SMP))   # ring upload, prompt Eval, first sample: what both loops start with
        plain_ms = med(lambda: c.SampleDecode(PROMPT, n, **SMP))
        step_ms = (plain_ms - head_ms) / (n - 1)
        out = dict(part="sample", int8=int8, layers=args.layers, ids=n, rows=K + 1, head_ms=round(head_ms, 3), sampled_ms=round(plain_ms, 2),
                   sampled_tok_s=round(n / plain_ms * 1e3, 1), step_ms=round(step_ms, 3))
        for name, corpus in (("replay", PROMPT + run), ("no_corpus", None)):
            res = {}

            def loop():
                ids, st, _ = c.SampleDecodeLookup(PROMPT, n, K, 3, 1, corpus, **SMP)
                assert ids == run and st["rows"] == K + 1, st
                res.update(st)
            ms = med(loop)
            pass_ms = (ms - head_ms) / res["passes"]
            out.update({f"{name}_passes": res["passes"], f"{name}_accepted": res["accepted"], f"{name}_ms": round(ms, 2), f"{name}_tok_s": round(n / ms * 1e3, 1),
                        f"{name}_pass_ms": round(pass_ms, 3)})
        out["pass_over_step"] = round(out["replay_pass_ms"] / step_ms, 3)
        # the route wins when ids per pass = 1 + mean accepted > pass time / step time
        out["break_even_accepted_per_pass"] = round(out["no_corpus_pass_ms"] / step_ms - 1, 3)
        emit(out)
        c.free()
        m.free()

if args.pods:
    args.parts = []
    P, ctx, n = args.pods, 256, 96
    prompts = [[PROMPT[0]] + [(t + 17 * i) % 32000 for t in PROMPT[1:]] for i in range(P)]
    past = [len(p) for p in prompts]
    for int8 in ([False, True] if args.int8 else [False]):
        m = model(ctx, int8)
        b = Batch(m, ctx, P)
        g = b.GreedyDecode(prompts, n + 1)
        first = [gi[0] for gi in g]
        replay = [t for p, gi in zip(prompts, g) for t in list(p) + gi]
        for K in (1, 3, 7):
            res = {}

            def loop(corpus):
                b.Prompt(prompts)
                _, _, st, _ = b.DecodeLookup(first, past, n, K, 3, 1, corpus)
                res.update(rows=st[0]["rows"], passes=max(s["passes"] for s in st), accepted=sum(s["accepted"] for s in st), pod_passes=sum(s["passes"] for s in st))

            def ticks():
                b.GreedyDecode(prompts, n + 1)
            head = lambda: b.Prompt(prompts)   # noqa: E731  (what all three start with)
            # alternating: replay, ticks, no corpus per repetition; medians per leg
            ts = {"head": [], "replay": [], "ticks": [], "no_corpus": []}
            legs = (("head", head), ("replay", lambda: loop(replay)), ("ticks", ticks), ("no_corpus", lambda: loop(None)))
            for _, fn in legs:
                fn()
            shape = {}
            for _ in range(args.reps):
                for name, fn in legs:
                    t0 = time.perf_counter(); fn(); ts[name].append((time.perf_counter() - t0) * 1e3)
                    if name in ("replay", "no_corpus"):
                        shape[name] = dict(res)
            md = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            R = shape["replay"]["rows"]
            if R == 1:
                emit(dict(part="pods", int8=int8, layers=args.layers, pods=P, draft_max=K, rows=1, note="no room for a second row: plain ticks"))
                continue
            tick_ms = (md["ticks"] - md["head"]) / n
            out = dict(part="pods", int8=int8, layers=args.layers, pods=P, draft_max=K, rows=R, pass_rows=P * R, ids_per_pod=n, tick_ms=round(tick_ms, 3),
                       ticks_tok_s=round(P * n / (md["ticks"] - md["head"]) * 1e3, 1))
            for name in ("replay", "no_corpus"):
                ms = md[name] - md["head"]
                out.update({f"{name}_passes": shape[name]["passes"], f"{name}_accepted_per_pod_pass": round(shape[name]["accepted"] / shape[name]["pod_passes"], 3),
                            f"{name}_pass_ms": round(ms / shape[name]["passes"], 3), f"{name}_tok_s": round(P * n / ms * 1e3, 1)})
            out["replay_is"] = "acceptance-1 ceiling (the corpus is the run itself), not a model result"
            out["pass_over_tick"] = round(out["no_corpus_pass_ms"] / tick_ms, 3)
            # the route wins when ids per pod and pass = 1 + mean accepted > pass time / tick time
            out["break_even_accepted_per_pod_pass"] = round(out["no_corpus_pass_ms"] / tick_ms - 1, 3)
            emit(out)
        b.free()
        m.free()

if "pass" in args.parts:
    N = 96   # ids per timed call: 12 full passes at R = 8
    for int8 in ([False, True] if args.int8 else [False]):
        for cached in (100, 1000):
            ctx = cached + 2 * N + 16
            m = model(ctx, int8)
            rng = np.random.default_rng(cached)
            prompt = [int(t) for t in rng.integers(0, 32000, cached)]
            c, first = prompt_state(m, ctx, prompt)
            g, _ = decode_greedy_resident(c, first, cached, N)
            step_ms = med(lambda: decode_greedy_resident(c, first, cached, N)) / N
            for R in ((2, 4) if int8 else (2, 4, 8)):
                res = {}

                def loop():
                    ids, _, st, _ = c.DecodeLookup(first, cached, N, R - 1, 3, 1, prompt[-8:] + [first] + g)
                    assert ids == g and st["rows"] == R, st
                    res.update(st)
                loop_ms = med(loop)
                b = Batch(m, ctx, R)
                pr, T = [prompt] * R, 48   # resident ticks of lh_batch_decode: the difference of two runs leaves the ticks alone (prompts and set-up cancel)
                tick_ms = (med(lambda: b.GreedyDecode(pr, 2 + T)) - med(lambda: b.GreedyDecode(pr, 2))) / T
                b.free()
                pass_ms = loop_ms / res["passes"]
                emit(dict(part="pass", int8=int8, layers=args.layers, cached=cached, rows=R, passes=res["passes"], ids=N, pass_ms=round(pass_ms, 3),
                          tick_of_R_pods_ms=round(tick_ms, 3), pass_over_tick=round(pass_ms / tick_ms, 3), step_ms=round(step_ms, 3),
                          pass_over_step=round(pass_ms / step_ms, 3)))
            c.free()
            m.free()

if "golden" in args.parts:
    for int8 in ([False, True] if args.int8 else [False]):
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "7b_seed1234_int8_ids.json" if int8 else "7b_seed1234_ids.json")))["ids"]
        K = 3 if int8 else 7
        m = model(128, int8)
        c, first = prompt_state(m, 128, PROMPT)
        n = 99
        exact = args.layers == 32
        greedy_ms = med(lambda: decode_greedy_resident(c, first, len(PROMPT), n))
        g, _ = decode_greedy_resident(c, first, len(PROMPT), n)
        assert not exact or [first] + g == gold
        out = dict(part="golden", int8=int8, layers=args.layers, ids=n, rows=K + 1, greedy_ms=round(greedy_ms, 2), greedy_tok_s=round(n / greedy_ms * 1e3, 1))
        for name, corpus in (("replay", PROMPT + [first] + g), ("no_corpus", None)):
            res = {}

            def loop():
                ids, _, st, _ = c.DecodeLookup(first, len(PROMPT), n, K, 3, 1, corpus)
                assert ids == g and st["rows"] == K + 1, st
                res.update(st)
            ms = med(loop)
            out.update({f"{name}_passes": res["passes"], f"{name}_accepted": res["accepted"], f"{name}_ms": round(ms, 2), f"{name}_tok_s": round(n / ms * 1e3, 1),
                        f"{name}_pass_ms": round(ms / res["passes"], 3)})
        # the route wins when ids per pass = 1 + mean accepted > pass time / step time
        out["break_even_accepted_per_pass"] = round(out["no_corpus_pass_ms"] / (greedy_ms / n) - 1, 3)
        emit(out)
        c.free()
        m.free()

if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
