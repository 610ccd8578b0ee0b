"""Draft-model speculative decoding (lh_llama_decode_draft) against plain greedy decode; results: profiles/draft_model.txt.
Synthetic LLaMA-7B fp32 target (seed 1234), its own block-int8 form (Model.QuantizeQ8 of the same weights) as the draft, ctx 128, the golden 8-token
prompt, 96 ids.  Host wall time of the calls (their synchronisations included); --reps repeats behind one warm-up of every leg, the legs alternating
in one process with plain lh_llama_decode_greedy; the table shows medians and the run-to-run spread (max - min).
  per draft_len 1 / 3 / 5 / 7: ms per pass, the measured acceptance (accepted / drafted, and accepted ids per pass), tokens/s, and the break-even
      accepted count per pass t_pass / t_step - 1 (t_step = the target's plain resident step);
  the parts, through the existing API: the draft's plain resident step (lh_llama_decode_greedy on the draft context) and the target's R-row verify
      pass (lh_llama_decode_lookup with the greedy run itself as corpus: every pass is full, time / passes);
  excess = t_pass - ((K + 1) * t_draft_step + t_verify) next to the spread of that sum; and, to say where an excess goes, a call of ONE id (one
      pass) against the cost of every further pass of the 96-id call.
The weights are synthetic: the acceptance of a block-int8 twin of RANDOM weights is what this run measured, not a model result.
--draft q4: the target's block-int4 form (Model.QuantizeQ4) as the draft instead: 20/36 of the int8 draft's bytes per drafted id.
usage: python tools/bench_draft_model.py [--layers 32] [--reps 3] [--ids 96] [--draft q8|q4] [--out profiles/draft_model.txt | profiles/draft_model_q4.txt]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from llama_go_amd.mlapi import PROMPT, SHAPES, DraftPair, decode_greedy_resident, load_product, make_hparams

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ids", type=int, default=96)
ap.add_argument("--ctx", type=int, default=128)
ap.add_argument("--out", default=None, help="default: profiles/draft_model.txt (--draft q8) or profiles/draft_model_q4.txt (--draft q4)")
ap.add_argument("--draft", choices=("q8", "q4"), default="q8")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "draft_model_q4.txt" if args.draft == "q4" else "draft_model.txt")
prod = load_product()
KS, n, ctx, past = (1, 3, 5, 7), args.ids, args.ctx, len(PROMPT)

kw = dict(SHAPES["7B"]); kw["layers"] = args.layers
target_model = prod.NewSyntheticModel(make_hparams(**kw, ctx=ctx), 1234)
draft_model = prod.NewSyntheticModel(make_hparams(**kw, ctx=ctx), 1234)
draft_model = draft_model.QuantizeQ4() if args.draft == "q4" else draft_model.QuantizeQ8()
DRAFT = "QuantizeQ4" if args.draft == "q4" else "QuantizeQ8"
DRAFT_FMT = "block-int4" if args.draft == "q4" else "block-int8"
pair = DraftPair(target_model, draft_model, ctx)
first = int(np.argmax(pair.target.Eval(PROMPT, 0)))
pair.draft.Eval(PROMPT, 0)
gold, _ = decode_greedy_resident(pair.target, first, past, n)
replay = PROMPT + [first] + gold
shape = {}


def leg_greedy():
    assert decode_greedy_resident(pair.target, first, past, n)[0] == gold


def leg_draft_step():
    decode_greedy_resident(pair.draft, first, past, n)


def leg_draft(K):
    ids, _, st, _ = pair.DecodeDraft(first, past, n, K)
    shape[("draft", K)] = dict(st, same_ids=ids == gold)


def leg_verify(K):
    ids, _, st, _ = pair.target.DecodeLookup(first, past, n, K, 3, 1, replay)
    shape[("verify", K)] = dict(st, same_ids=ids == gold)


def leg_one(K):     # one id = one full-width pass with nothing drafted: what a call costs beyond its passes
    pair.DecodeDraft(first, past, 1, K)


legs = [("greedy", leg_greedy), ("draft_step", leg_draft_step)]
for K in KS:
    legs += [(f"draft{K}", lambda K=K: leg_draft(K)), (f"verify{K}", lambda K=K: leg_verify(K)), (f"one{K}", lambda K=K: leg_one(K))]
for _, fn in legs:      # warm-up: plans, kernel attributes, the graph captures of the resident and lookup loops
    fn()
ts = {name: [] for name, _ in legs}
for _ in range(args.reps):
    for name, fn in legs:
        t0 = time.perf_counter(); fn(); ts[name].append((time.perf_counter() - t0) * 1e3)
    # every leg starts from the prompt's rows [0, past), which no leg overwrites; the draft's rows behind them are rewritten by each leg itself
med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
spr = {k: max(v) - min(v) for k, v in ts.items()}

t_step, t_dstep = med["greedy"] / n, med["draft_step"] / n
out = ["# tools/bench_draft_model.py: synthetic 7B fp32 target (%d layers), its %s twin as draft, ctx %d, %d ids, %d repeats (median, spread = max - min)" % (args.layers, DRAFT, ctx, n, args.reps),
       "# acceptance on RANDOM weights is an artefact of the synthetic model, not a model result; there is no speed-up gate",
       "plain greedy (target): %.3f ms/step  %.1f tok/s  (spread of the %d-id run %.2f ms)" % (t_step, 1e3 / t_step, n, spr["greedy"]),
       "draft plain resident step (%s twin): %.3f ms/step  %.1f tok/s  (spread of the run %.2f ms)" % (DRAFT_FMT, t_dstep, 1e3 / t_dstep, spr["draft_step"]),
       "",
       "draft_len rows passes  ms/pass  accepted/drafted  acc/pass  tok/s   vs greedy  break-even acc/pass | t_verify(R)  (K+1)*t_dstep  excess    spread of the parts  same ids"]
rows = []
for K in KS:
    d, v = shape[("draft", K)], shape[("verify", K)]
    t_pass = med[f"draft{K}"] / d["passes"]
    t_ver = med[f"verify{K}"] / v["passes"]
    parts = (K + 1) * t_dstep + t_ver
    part_spread = (K + 1) * spr["draft_step"] / n + spr[f"verify{K}"] / v["passes"]
    tok_s = n / med[f"draft{K}"] * 1e3
    # a call of ONE id runs one pass: the rest of its wall time is what every call pays once (state set-up, the host's looks, the copies back)
    call_ms = (med[f"draft{K}"] - med[f"one{K}"]) / max(d["passes"] - 1, 1)      # ms per pass with the per-call cost taken off
    r = dict(draft_len=K, rows=d["rows"], passes=d["passes"], ms_per_pass=round(t_pass, 3), drafted=d["drafted"], accepted=d["accepted"],
             acceptance=round(d["accepted"] / max(d["drafted"], 1), 4), accepted_per_pass=round(d["accepted"] / d["passes"], 3), tok_s=round(tok_s, 1),
             speedup=round(tok_s * t_step / 1e3, 3), break_even_accepted_per_pass=round(t_pass / t_step - 1, 3), t_verify_ms=round(t_ver, 3),
             draft_steps_ms=round((K + 1) * t_dstep, 3), excess_ms=round(t_pass - parts, 3), parts_spread_ms=round(part_spread, 3),
             pass_spread_ms=round(spr[f"draft{K}"] / d["passes"], 3), one_id_call_ms=round(med[f"one{K}"], 3), ms_per_further_pass=round(call_ms, 3),
             excess_further_pass_ms=round(call_ms - parts, 3), verify_passes=v["passes"], same_ids=bool(d["same_ids"] and v["same_ids"]))
    rows.append(r)
    out.append("%9d %4d %6d %8.3f  %6d/%-6d %4.2f  %8.3f %7.1f %8.3fx %12.3f            | %10.3f %14.3f %8.3f  %10.3f           %s"
               % (K, r["rows"], r["passes"], t_pass, r["accepted"], r["drafted"], r["acceptance"], r["accepted_per_pass"], tok_s, r["speedup"],
                  r["break_even_accepted_per_pass"], t_ver, (K + 1) * t_dstep, r["excess_ms"], part_spread, r["same_ids"]))
out.append("")
out.append("a call of ONE id (one pass, nothing drafted) and the cost of every further pass = (t_call - t_one) / (passes - 1); its excess over the parts:")
for r in rows:
    out.append("draft_len %d: one-id call %.3f ms, a further pass %.3f ms, excess %.3f ms" % (r["draft_len"], r["one_id_call_ms"], r["ms_per_further_pass"], r["excess_further_pass_ms"]))
out.append("")
out += [json.dumps(dict(part="draft_model", layers=args.layers, ctx=ctx, ids=n, reps=args.reps, greedy_ms_per_step=round(t_step, 4),
                        draft_ms_per_step=round(t_dstep, 4), **r)) for r in rows]
try:    # register / scratch / spill metadata of the new kernel (tools/isa_check.py; host only)
    isa = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), "--filter", "k_draft_model"], capture_output=True, text=True).stdout
    out += ["", "# tools/isa_check.py --filter k_draft_model"] + isa.strip().splitlines()
except OSError as e:
    out.append(f"# tools/isa_check.py not run: {e}")
text = "\n".join(out) + "\n"
print(text)
with open(args.out, "w") as f:
    f.write(text)
pair.free()
draft_model.free()
target_model.free()
