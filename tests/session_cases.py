"""The trigger table and the scripts of the session tests (tests/session_ref.py runs them; no GPU needed to import).

TRIGGERS lists every place in csrc/plan.hip, score.hip, abi.hip and comm.hip that re-allocates something or drops / re-keys a captured graph (found by
reading every call of the grow helper `grow(`, every `hipFree(`, every generation counter `*_gen` and every key struct of a CapturedGraph in those files).  Each row says what a captured graph must do behind it:
  recapture   the graph holds what moved: the next graph-run step must record launches again (CAPTURE), the one after it none (REPLAY)
  keep        nothing a graph holds moved: the next graph-run step must still REPLAY
and names the scripts whose steps fire it (Step.fires; "name>Call" where the graph that must notice belongs to another call than the next one: a lookup
run that grows the scratch under the captured TICK).  tests/test_session_cpu.py holds table and scripts to each other.

Scripts are static: every token id and position is written down here, no step uses an id an earlier step produced (a decode run that "continues" restarts
from a fixed first token at the position the run before it reached - a valid call, and all that matters to the caches).  Shapes are the smallest at
which the triggers exist: `small` (embd 1024, head size 128: split-K, the plane GEMM and the split-T partials exist) and `tiny` where only row counts matter.
"""
from session_ref import CAPTURE, DECODE_RE, DETOUR, EAGER, ESSENTIAL, KERNEL_RE, REPLAY, ROWS_RE, Script, Step, swap_positions, toks

VOCAB = {"tiny": 512, "small": 2048}
WEIGHTS = ("f32", "q8")

RECAPTURE, KEEP = "recapture", "keep"

# name -> (where, what fires it, what a captured graph must do behind it, scripts that fire it or the reason none does)
TRIGGERS = {
    "plan_ensure_rows": ("plan.hip plan_ensure_rows", "an Eval / Score / Verify / feed pass of more rows than the plan's scratch holds: every scratch buffer, the "
                         "s3 planes and tokens_dev move, scratch_gen grows (in every key: DecodeKey, TickKey, Spec::Key, BatchSpec::Key)", RECAPTURE,
                         ("solo.growing_prompts", "solo.resident_around_detours", "solo.speculation_interleaved", "batch.ticks_around_feeds", "batch.lookup_among_ticks")),
    "ensure_out_tokens": ("plan.hip ensure_out_tokens", "a resident run of more than 4096 ids: out_tokens_dev moves, out_gen grows (DecodeKey of the ADV and SMP slots only)", RECAPTURE,
                          ("solo.more_than_4096_ids",)),
    "solo_sampler_variant": ("plan.hip decode_sample", "topK crosses 64: the captured sampled step holds the kernel variant, smp_gen grows (DecodeKey of the SMP slots)", RECAPTURE,
                             ("solo.sampler_reconfiguration",)),
    "solo_ring_growth": ("plan.hip decode_sample", "a ring larger than ring_cap: ring_dev moves, smp_gen grows (DecodeKey of the SMP slots); the sampled verify pass compares Spec::Key::ring", RECAPTURE,
                         ("solo.sampler_reconfiguration",)),
    "solo_ring_smaller": ("plan.hip decode_sample", "a ring smaller than ring_cap: ring_dev stays, the ring is re-initialised in place", KEEP,
                          ("solo.sampler_reconfiguration",)),
    "plan_embeddings": ("plan.hip plan_embeddings", "embedding output of more rows than emb holds: emb moves; no graph holds it", KEEP, ("solo.resident_around_detours",)),
    "other_plan_rows": ("plan.hip plan_ensure_rows on the context's OTHER plan", "llama_Eval runs on the plan the fused-graph matcher finds, the resident calls on the "
                        "plan of lh_llama_create: an n-row Eval grows the first one's scratch and leaves the resident graphs alone (and the other way round)", KEEP,
                        ("solo.resident_around_detours",)),
    "score_dev": ("score.hip lh_llama_score", "a Score of more rows than score_dev holds: score_dev moves; no graph holds it", KEEP, ("solo.resident_around_detours",)),
    "verify_pass": ("plan.hip lh_llama_verify", "the speculative state of a plan is created beside live decode graphs (spec_ensure); nothing they hold moves", KEEP,
                    ("solo.resident_around_detours",)),
    "eval_cache": ("host/llamago.cpp llama_Eval (llamago_KeepDecodeGraph)", "the host mirror keeps the one-token ml graph between Evals and moves its position: an n-row "
                   "Eval between two one-token Evals must not leave the kept graph on the old scratch", RECAPTURE, ("solo.growing_prompts",)),
    "ensure_splitk": ("plan.hip ensure_splitk (grow)", "a split-K launch of more partial products than the context's buffer holds: splitk moves, splitk_gen "
                      "grows (the batch tick and both verify passes compare it; solo decode graphs hold no split-K buffer)", RECAPTURE,
                      ("solo.growing_prompts", "batch.ticks_around_feeds")),
    "ensure_xs3": ("plan.hip ensure_xs3", "block-int8, a prompt from 89 rows on: the context's bf16 planes move, splitk_gen grows", RECAPTURE,
                   ("solo.growing_prompts", "batch.ticks_around_feeds")),
    "prefill_scratch": ("plan.hip attention_gemm / attention_flash (scores, vt, part, fa_part)", "prompt attention scratch grows with the row count; only launches of "
                        "32 rows and more without a row table use it, which no capture contains", KEEP, ("solo.growing_prompts",)),
    "ensure_staging": ("abi.hip ensure_staging", "the pinned staging buffer grows; uploads from it are enqueued outside every capture", KEEP, ("solo.growing_prompts",)),
    "ensure_rope_table": ("abi.hip ensure_rope_table", "a context with a longer window appears on the device: a larger cos/sin table is built, the old one stays "
                          "allocated for the plans that hold its address", KEEP, ("solo.longer_window_appears",)),
    "other_object_freed": ("plan.hip plan_destroy / batch_free", "another context or batch of the same model is created, used and freed: its buffers return to the "
                           "allocator while the long-lived object's graphs stay valid", KEEP, ("solo.longer_window_appears", "batch.batches_come_and_go")),
    "spec_key_R": ("plan.hip spec_pass (Spec::Key::R, warm bit R)", "lookup passes of another row count: the first one runs eagerly, the graph is re-captured", RECAPTURE,
                   ("solo.speculation_interleaved",)),
    "spec_key_lookup": ("plan.hip spec_pass (Spec::Key::lp) / spec_ensure corpus", "another n-gram range or a corpus: the accept kernel holds them by value, the corpus buffer moves",
                        RECAPTURE, ("solo.speculation_interleaved",)),
    "spec_key_sampled": ("plan.hip spec_pass (Spec::Key::smp, smp_small, ring, out)", "greedy passes after sampled ones and back: other launches, other output offset",
                         RECAPTURE, ("solo.speculation_interleaved",)),
    "spec_trace_growth": ("plan.hip spec_ensure / batch_spec_ensure (trace)", "a lookup run of more passes than the trace buffer holds (4096): the buffer moves, the keys' trace "
                          "differs", RECAPTURE, "not covered: needs a lookup run of more than 4096 ids per call, which no script's window allows in a few seconds"),
    "batch_scratch_gen": ("plan.hip batch_tick_unchecked (TickKey::scratch_gen)", "a feed grows pod 0's scratch to FEED_PASS_ROWS, or a pod's own Eval (a feed of "
                          "LLAMAHIP_FEED_SOLO_MIN rows and more) grows that pod's: the sum of the pods' scratch_gen moves", RECAPTURE,
                          ("batch.ticks_around_feeds", "batch.lookup_among_ticks")),
    "feed_dev": ("plan.hip batch_feed (feed_dev, feed_part)", "a feed whose tables need more bytes than feed_dev holds; only the feed's own eager passes read it", KEEP,
                 ("batch.ticks_around_feeds",)),
    "batch_sampling": ("plan.hip batch_tick_unchecked (TickKey::sampling)", "lh_batch_set_sampler on or off: the tick ends in another kernel", RECAPTURE,
                       ("batch.sampler_on_off_on", "batch.lookup_among_ticks")),
    "batch_ring_growth": ("plan.hip lh_batch_set_sampler", "a ring larger than ring_cap: ring_dev moves, Batch::smp_gen grows (TickKey::smp_gen)", RECAPTURE, ("batch.sampler_on_off_on",)),
    "batch_sampler_variant": ("plan.hip lh_batch_set_sampler", "topK crosses 64: Batch::smp_gen grows (TickKey::smp_gen)", RECAPTURE, ("batch.sampler_on_off_on",)),
    "batch_ring_smaller": ("plan.hip lh_batch_set_sampler", "a ring smaller than ring_cap, same variant: every ring re-initialised in place with the new size", KEEP,
                           ("batch.sampler_on_off_on",)),
    "env_sample_per_pod": ("plan.hip batch_tick_unchecked (TickKey::per_pod)", "LLAMAHIP_SAMPLE_PER_POD changes between two ticks", RECAPTURE, ("batch.sampler_on_off_on",)),
    "batch_shared": ("plan.hip batch_tick_unchecked (TickKey::shared)", "the block table goes from no block to some block (a fork) or back (LLAMAHIP_SHARE_ROW_ATTN)", RECAPTURE,
                     ("batch.fork_and_unfork",)),
    "share_table": ("plan.hip share_prepare (share_sent)", "a member leaves its group or a group re-forms: the table is re-sent in front of the tick, the captured tick "
                    "reads it from a fixed address", KEEP, ("batch.fork_and_unfork",)),
    "env_share_qb": ("plan.hip batch_tick_unchecked (TickKey::share_qb)", "LLAMAHIP_SHARE_QB changes between two shared ticks", RECAPTURE, ("batch.fork_and_unfork",)),
    "env_feed_row_attn": ("plan.hip batch_feed", "LLAMAHIP_FEED_ROW_ATTN=1 for one feed: the per-row kernels, the same bytes; feeds are never captured", KEEP,
                          ("batch.ticks_around_feeds",)),
    "batch_spec_key_R": ("plan.hip batch_spec_pass (BatchSpec::Key::R, warm bit pods x R - 1)", "lookup passes of another pods x R", RECAPTURE, ("batch.lookup_among_ticks",)),
    "batch_spec_key_sampled": ("plan.hip batch_spec_pass (BatchSpec::Key::smp, small_k, ss, ring, ring_cap)", "sampled passes after greedy ones and back", RECAPTURE,
                               ("batch.lookup_among_ticks",)),
    "batch_x_in_out": ("plan.hip batch_tick_unchecked (TickKey::x_in, x_out)", "a layer shard's tick gets another residual buffer", RECAPTURE,
                       "not covered: needs ranks (only lh_pipeline_* hands a tick residual buffers)"),
    "pipeline_rows_cap": ("comm.hip lh_pipeline (rows_cap)", "the grouped re-allocation of a pipeline's row buffers", RECAPTURE, "not covered: needs ranks"),
    "arena": ("abi.hip ensure_arena", "the node path's tensor arena grows; the node path captures nothing", KEEP,
              "not covered: no graph exists on the node path (tests/test_gpu_node_ops.py runs it)"),
}


def E(call, trace=None, fires=(), rx=KERNEL_RE, **kw):
    extra = {k: kw.pop(k) for k in ("env", "equals", "twin", "note") if k in kw}
    return Step(call, kw, ESSENTIAL, trace, tuple(fires), rx, **extra)


def D(call, trace=None, fires=(), rx=KERNEL_RE, **kw):
    extra = {k: kw.pop(k) for k in ("env", "equals", "twin", "note") if k in kw}
    return Step(call, kw, DETOUR, trace, tuple(fires), rx, **extra)


# ---- solo ------------------------------------------------------------------------------------------------------------------------------------------------
def growing_prompts(weights):
    """One-token Evals (the G_STEP graph through the host mirror's kept ml graph) around prompts of 20, 70 and 200 (block-int8: 100) rows, each a detour at a
    rewound position: every growth moves the scratch, the last one crosses into the tile GEMM (fp32 193+: split-K; block-int8 89+: the xs3 planes)."""
    V = VOCAB["small"]
    big = 200 if weights == "f32" else 100
    last = ("plan_ensure_rows", "ensure_staging", "prefill_scratch") + (("ensure_splitk",) if weights == "f32" else ("ensure_xs3",))
    s = [E("Eval", EAGER, tokens=toks(3, 1, V), past=0),
         E("Eval", CAPTURE, tokens=[11], past=3, rx=DECODE_RE), E("Eval", REPLAY, tokens=[12], past=4, rx=DECODE_RE),
         D("Eval", EAGER, ("plan_ensure_rows", "eval_cache"), tokens=toks(20, 2, V), past=5),
         E("Eval", CAPTURE, tokens=[13], past=5, rx=DECODE_RE), E("Eval", REPLAY, tokens=[14], past=6, rx=DECODE_RE),
         D("Eval", EAGER, ("plan_ensure_rows", "prefill_scratch"), tokens=toks(70, 3, V), past=7),
         E("Eval", CAPTURE, tokens=[15], past=7, rx=DECODE_RE), E("Eval", REPLAY, tokens=[16], past=8, rx=DECODE_RE),
         D("Eval", EAGER, last, tokens=toks(big, 4, V), past=9),
         E("Eval", CAPTURE, tokens=[17], past=9, rx=DECODE_RE), E("Eval", REPLAY, tokens=[18], past=10, rx=DECODE_RE),
         E("CacheImage", pos=11)]
    return Script("solo.growing_prompts", "solo", "small", 256, tuple(s), doc=growing_prompts.__doc__)


def resident_around_detours(weights):
    """The resident greedy loop (G_ADV1 / G_ADVN) continuing behind detours at the end position.  A context has TWO plans over one cache: llama_Eval runs on
    the plan the fused-graph matcher finds, the resident calls (Decode, Score, Verify, the lookup and sampled loops) on the plan of lh_llama_create.  So only
    the resident calls move what the resident graphs hold: the first Verify pass (4 rows) and the Scores of 64 and 66 rows grow that plan's scratch
    (re-capture); a Score of 3 rows grows score_dev alone, a second Verify pass creates nothing, and a 70-row Eval with embedding output grows the OTHER
    plan's scratch and emb (replay, all three).  Embedding output has no switch back in the host mirror: it stays on, and the fresh twin, which never had
    it, must still agree."""
    V = VOCAB["small"]
    s = [E("Eval", EAGER, tokens=toks(6, 1, V), past=0),
         E("Decode", CAPTURE, first=21, past=6, n=10, rx=DECODE_RE), E("Decode", REPLAY, first=22, past=16, n=10, rx=DECODE_RE),
         D("Verify", EAGER, ("plan_ensure_rows",), tokens=toks(4, 3, V), past=26),
         E("Decode", CAPTURE, first=23, past=26, n=10, rx=DECODE_RE), E("Decode", REPLAY, first=24, past=36, n=10, rx=DECODE_RE),
         D("Score", EAGER, ("score_dev",), tokens=toks(3, 6, V), past=46),
         E("Decode", REPLAY, first=25, past=46, n=10, rx=DECODE_RE),
         D("Score", EAGER, ("plan_ensure_rows", "score_dev"), tokens=toks(64, 2, V), past=56),
         E("Decode", CAPTURE, first=26, past=56, n=10, rx=DECODE_RE), E("Decode", REPLAY, first=27, past=66, n=10, rx=DECODE_RE),
         D("Verify", EAGER, ("verify_pass",), tokens=toks(4, 7, V), past=76),
         E("Decode", REPLAY, first=28, past=76, n=10, rx=DECODE_RE),
         D("EmbeddingEval", EAGER, ("plan_embeddings", "other_plan_rows"), tokens=toks(70, 4, V), past=86),
         E("Decode", REPLAY, first=29, past=86, n=10, rx=DECODE_RE),
         D("Score", EAGER, ("plan_ensure_rows", "score_dev"), tokens=toks(66, 5, V), past=96),
         E("Decode", CAPTURE, first=30, past=96, n=10, rx=DECODE_RE), E("Decode", REPLAY, first=31, past=106, n=10, rx=DECODE_RE),
         E("CacheImage", pos=116)]
    return Script("solo.resident_around_detours", "solo", "small", 256, tuple(s), doc=resident_around_detours.__doc__)


def sampler_reconfiguration(weights):
    """The resident sampled loop (G_SMP1 / G_SMPN) through topK 40 -> 100 (the kernel variant flips) -> a ring of 256 (ring_dev grows) -> a ring of 32 (smaller
    than the capacity) -> the first configuration again, whose ids must repeat the very first run byte for byte.  SampleDecode's ring is the window (64), as
    in the reference; the ring size of a solo context moves only through SampleDecodeLookup, so those two steps are lookup runs."""
    V = VOCAB["tiny"]
    p = toks(8, 1, V)
    first = dict(prompt=p, n=24, topK=40, seed=7)
    s = [E("SampleDecode", CAPTURE, rx=DECODE_RE, **first), E("SampleDecode", REPLAY, rx=DECODE_RE, equals=0, **first),
         E("SampleDecode", CAPTURE, ("solo_sampler_variant",), rx=DECODE_RE, prompt=p, n=24, topK=100, seed=7),
         E("SampleDecode", REPLAY, rx=DECODE_RE, equals=2, prompt=p, n=24, topK=100, seed=7),
         E("SampleDecodeLookup", EAGER, ("solo_ring_growth", "solo_sampler_variant"), rx=ROWS_RE, prompt=p, n=24, draft_max=3, ring=256, topK=40, seed=7),
         E("SampleDecode", CAPTURE, rx=DECODE_RE, equals=0, **first), E("SampleDecode", REPLAY, rx=DECODE_RE, equals=0, **first),
         E("SampleDecodeLookup", REPLAY, ("solo_ring_smaller",), rx=ROWS_RE, prompt=p, n=24, draft_max=3, ring=32, topK=40, seed=7),
         E("SampleDecode", REPLAY, rx=DECODE_RE, equals=0, **first),
         E("CacheImage", pos=31)]
    return Script("solo.sampler_reconfiguration", "solo", "tiny", 64, tuple(s), doc=sampler_reconfiguration.__doc__)


def speculation_interleaved(weights):
    """Lookup-draft runs of R = 4, a plain resident run, R = 8 (block-int8: 2, its limit is 4 rows) with another n-gram range, a corpus, a sampled lookup run,
    R = 4 again (the prompt goes in as a Score of 12 rows on the resident plan, so that neither R = 8 nor the sampled run's 10-row prompt grows its scratch: the
    captures behind them are the pass key's alone), and a 70-row Score detour between two R = 4 runs (scratch_gen moves under the pass graph; an Eval would not do: it runs on
    the context's other plan, see resident_around_detours)."""
    V = VOCAB["small"]
    k2 = 7 if weights == "f32" else 1
    s = [E("Score", EAGER, tokens=toks(12, 1, V), past=0),
         E("DecodeLookup", EAGER, rx=ROWS_RE, first=31, past=12, n=16, draft_max=3), E("DecodeLookup", REPLAY, rx=ROWS_RE, first=32, past=28, n=16, draft_max=3),
         E("Decode", CAPTURE, rx=DECODE_RE, first=33, past=44, n=8),
         E("DecodeLookup", EAGER, ("spec_key_R", "spec_key_lookup"), rx=ROWS_RE, first=34, past=52, n=16, draft_max=k2, ngram_max=4, ngram_min=2),
         E("DecodeLookup", REPLAY, rx=ROWS_RE, first=35, past=68, n=16, draft_max=k2, ngram_max=4, ngram_min=2),
         E("DecodeLookup", CAPTURE, ("spec_key_lookup",), rx=ROWS_RE, first=36, past=84, n=16, draft_max=k2, ngram_max=4, ngram_min=2, corpus=toks(48, 9, V)),
         E("DecodeLookup", REPLAY, rx=ROWS_RE, first=37, past=100, n=16, draft_max=k2, ngram_max=4, ngram_min=2, corpus=toks(48, 9, V)),
         E("SampleDecodeLookup", CAPTURE, ("spec_key_sampled", "spec_key_R"), rx=ROWS_RE, prompt=toks(10, 2, V), n=16, draft_max=3, ring=64, topK=40, seed=7),
         E("DecodeLookup", CAPTURE, ("spec_key_sampled",), rx=ROWS_RE, first=38, past=25, n=16, draft_max=3),
         E("DecodeLookup", REPLAY, rx=ROWS_RE, first=39, past=41, n=16, draft_max=3),
         D("Score", EAGER, ("plan_ensure_rows",), tokens=toks(70, 3, V), past=57),
         E("DecodeLookup", CAPTURE, rx=ROWS_RE, first=40, past=57, n=16, draft_max=3),
         E("DecodeLookup", REPLAY, rx=ROWS_RE, first=41, past=73, n=16, draft_max=3),
         E("Decode", CAPTURE, rx=DECODE_RE, first=42, past=89, n=8), E("Decode", REPLAY, rx=DECODE_RE, first=43, past=97, n=8),
         E("CacheImage", pos=105)]
    return Script("solo.speculation_interleaved", "solo", "small", 256, tuple(s), doc=speculation_interleaved.__doc__)


N_LONG = 4100


def more_than_4096_ids(weights):
    """One resident greedy run of 4100 ids in a window of 64 with KeepCount 8 (it swaps context every 28 steps), between short runs: the output list grows past
    4096 ids (ensure_out_tokens), which drops only the greedy and sampled slots.  The eager twin makes the ids in two runs of 2050, the second one starting
    from the first one's last id at the position the swaps left it.  The prompt goes in as a Score of 32 rows: it runs on the resident plan (an Eval would not),
    so that no swap's re-fed run of 28 rows grows that plan's scratch in the middle of the long run."""
    V = VOCAB["tiny"]
    ctx, keep = 64, 8
    end = swap_positions(52, N_LONG, ctx, keep)
    s = [E("SetKeepCount", keep=keep), E("Score", EAGER, tokens=toks(32, 1, V), past=0),
         E("Decode", CAPTURE, rx=DECODE_RE, first=51, past=32, n=10), E("Decode", REPLAY, rx=DECODE_RE, first=52, past=42, n=10),
         E("Decode", CAPTURE, ("ensure_out_tokens",), rx=DECODE_RE, first=53, past=52, n=N_LONG,
           twin=Step("DecodeSplit", dict(first=53, past=52, counts=(N_LONG // 2, N_LONG - N_LONG // 2), keep=keep))),
         E("Decode", REPLAY, rx=DECODE_RE, first=54, past=end, n=10),
         E("CacheImage", pos=swap_positions(end, 10, ctx, keep))]
    return Script("solo.more_than_4096_ids", "solo", "tiny", ctx, tuple(s), doc=more_than_4096_ids.__doc__)


def longer_window_appears(weights):
    """Resident decode on a window of 64; a context of 512 positions of the same model appears and evaluates one row near its end (the device's RoPE table
    grows where no longer window was seen before; the old table stays for the plans that hold it), decode goes on, the second context goes, decode goes on."""
    V = VOCAB["tiny"]
    s = [E("Eval", EAGER, tokens=toks(8, 1, V), past=0),
         E("Decode", CAPTURE, rx=DECODE_RE, first=61, past=8, n=10), E("Decode", REPLAY, rx=DECODE_RE, first=62, past=18, n=10),
         D("OpenOther", None, ("ensure_rope_table",), ctx=512, tokens=[63], past=510),
         E("Decode", REPLAY, rx=DECODE_RE, first=64, past=28, n=10),
         D("CloseOther", None, ("other_object_freed",)),
         E("Decode", REPLAY, rx=DECODE_RE, first=65, past=38, n=10),
         E("CacheImage", pos=48)]
    return Script("solo.longer_window_appears", "solo", "tiny", 64, tuple(s), doc=longer_window_appears.__doc__)


# ---- batch (4 pods) --------------------------------------------------------------------------------------------------------------------------------------
PODS = 4


def _prompts(V, lens, seed=1):
    return [toks(n, seed + i, V) for i, n in enumerate(lens)]


def ticks_around_feeds(weights):
    """Ticks of four pods around feeds: 24 rows to one pod (pod 0's scratch grows to the 64 rows of a feed pass), 60 rows to three pods (full 64-row passes: the
    context's split-K buffer grows, which the captured tick compares), 60 rows to all four on the per-row attention kernels (feed_dev grows; nothing the tick
    holds moves), and 130 rows to one pod - an Eval of its own on that pod's plan (its scratch_gen moves and, through the tile GEMM, split-K or the planes)."""
    V = VOCAB["small"]
    big = ("plan_ensure_rows", "batch_scratch_gen") + (("ensure_splitk",) if weights == "f32" else ("ensure_xs3",))
    s = [E("Prompt", EAGER, prompts=_prompts(V, (5, 7, 6, 9))),
         E("Tick", EAGER), E("Tick", CAPTURE), E("Tick", REPLAY),                                                        # -> 8, 10, 9, 12
         E("Feed", EAGER, ("plan_ensure_rows", "batch_scratch_gen", "feed_dev"), tokens=[[], toks(24, 5, V), [], []], past=[0, 10, 0, 0]),
         E("Tick", CAPTURE), E("Tick", REPLAY),                                                                          # -> 10, 36, 11, 14
         E("Feed", EAGER, ("feed_dev", "ensure_splitk"), tokens=[toks(60, 6, V), toks(60, 7, V), toks(60, 8, V), []], past=[10, 36, 11, 0]),
         E("Tick", CAPTURE), E("Tick", REPLAY),                                                                          # -> 72, 98, 73, 16
         E("Feed", EAGER, ("feed_dev", "env_feed_row_attn"), tokens=[toks(60, 10 + i, V) for i in range(4)], past=[72, 98, 73, 16],
           env=(("LLAMAHIP_FEED_ROW_ATTN", "1"),)),
         E("Tick", REPLAY, env=(("LLAMAHIP_FEED_ROW_ATTN", None),)),                                                     # -> 133, 159, 134, 77
         E("Feed", EAGER, big, tokens=[[], [], [], toks(130, 9, V)], past=[0, 0, 0, 77]),
         E("Tick", CAPTURE), E("Tick", REPLAY),                                                                          # -> 135, 161, 136, 209
         E("CacheImage", pos=[135, 161, 136, 209])]
    return Script("batch.ticks_around_feeds", "batch", "small", 384, tuple(s), PODS, ticks_around_feeds.__doc__)


def sampler_on_off_on(weights):
    """Greedy ticks, a sampler of topK 40 and ring 64, topK 100 with a ring of 128, greedy again, a sampler set and at once replaced (a detour), the first
    configuration again with a ring smaller than the capacity, and LLAMAHIP_SAMPLE_PER_POD switched on and off between ticks (the same bytes as the unswitched
    twins).  Rings, ring positions and draw counters are read at every step."""
    s = [E("Prompt", EAGER, prompts=_prompts(VOCAB["small"], (5, 7, 6, 9))),
         E("Tick", EAGER), E("Tick", CAPTURE), E("Tick", REPLAY),
         E("SetSampler", None, ("batch_sampling", "batch_ring_growth"), topK=40, seed=5, ring=64),
         E("Tick", CAPTURE), E("Tick", REPLAY), E("SamplerState"),
         E("SetSampler", None, ("batch_ring_growth", "batch_sampler_variant"), topK=100, seed=6, ring=128),
         E("Tick", CAPTURE), E("Tick", REPLAY), E("SamplerState"),
         E("ClearSampler", None, ("batch_sampling",)),
         E("Tick", CAPTURE), E("Tick", REPLAY),
         D("SetSampler", None, (), topK=100, seed=9, ring=128),
         E("SetSampler", None, ("batch_sampling", "batch_sampler_variant"), topK=40, seed=5, ring=64),
         E("Tick", CAPTURE), E("Tick", REPLAY), E("SamplerState"),
         E("SetSampler", None, ("batch_ring_smaller",), topK=40, seed=8, ring=32),
         E("Tick", REPLAY), E("SamplerState"),
         E("Tick", CAPTURE, ("env_sample_per_pod",), env=(("LLAMAHIP_SAMPLE_PER_POD", "1"),)), E("Tick", REPLAY),
         E("Tick", CAPTURE, ("env_sample_per_pod",), env=(("LLAMAHIP_SAMPLE_PER_POD", None),)), E("Tick", REPLAY), E("SamplerState"),
         E("CacheImage", pos=[5 + 16, 7 + 16, 6 + 16, 9 + 16])]
    return Script("batch.sampler_on_off_on", "batch", "small", 256, tuple(s), PODS, sampler_on_off_on.__doc__)


def fork_and_unfork(weights):
    """A prefix of 300 keys (two full 128-key chunks) forked to 3 of 4 pods in a window of 384: ticks on the shared kernel; one member is set below the shared
    length and leaves (the table is re-sent, the captured tick stays); the source forks to both again at its new length; then LLAMAHIP_SHARE_ROW_ATTN and LLAMAHIP_SHARE_QB are
    switched between ticks (re-capture; the same bytes as the unswitched twins)."""
    V = VOCAB["small"]
    s = [E("Feed", EAGER, tokens=[toks(300, 1, V), [1], [2], [3]], past=[0, 0, 0, 0]),
         E("Fork", src=0, dst=[1, 2], n_pos=300),
         E("Set", tokens=[71, 72, 73, 74], past=[300, 300, 300, 1]),
         E("Tick", EAGER, ("batch_shared",)), E("Tick", CAPTURE), E("Tick", REPLAY),                                      # -> 303, 303, 303, 4
         E("Set", None, ("share_table",), tokens=[75, 76, 77, 78], past=[303, 200, 303, 4]),
         E("Tick", REPLAY), E("Tick", REPLAY),                                                                           # -> 305, 202, 305, 6
         E("Fork", None, ("share_table",), src=0, dst=[1, 2], n_pos=305),
         E("Set", tokens=[79, 80, 81, 82], past=[305, 305, 305, 6]),
         E("Tick", REPLAY), E("Tick", REPLAY),                                                                           # -> 307, 307, 307, 8
         E("Tick", CAPTURE, ("batch_shared",), env=(("LLAMAHIP_SHARE_ROW_ATTN", "1"),)), E("Tick", REPLAY),
         E("Tick", CAPTURE, ("batch_shared",), env=(("LLAMAHIP_SHARE_ROW_ATTN", None),)), E("Tick", REPLAY),
         E("Tick", CAPTURE, ("env_share_qb",), env=(("LLAMAHIP_SHARE_QB", "2"),)), E("Tick", REPLAY),
         E("Tick", CAPTURE, ("env_share_qb",), env=(("LLAMAHIP_SHARE_QB", None),)), E("Tick", REPLAY),                    # -> 315, 315, 315, 16
         E("CacheImage", pos=[315, 315, 315, 16])]
    return Script("batch.fork_and_unfork", "batch", "small", 384, tuple(s), PODS, fork_and_unfork.__doc__)


def lookup_among_ticks(weights):
    """Lookup-draft passes of 4 pods x R rows among ticks: R = 2, ticks, R = 4 (pod 0's scratch grows under the captured tick), a sampler, sampled passes, the
    sampler cleared, R = 2 again."""
    V = VOCAB["small"]
    p0 = [10, 12, 11, 13]
    at = lambda k: [p + k for p in p0]   # noqa: E731
    s = [E("Prompt", EAGER, prompts=_prompts(V, p0)),
         E("DecodeLookup", EAGER, first=[91, 92, 93, 94], past=at(0), n=8, draft_max=1), E("DecodeLookup", REPLAY, first=[95, 96, 97, 98], past=at(8), n=8, draft_max=1),
         E("Set", tokens=[101, 102, 103, 104], past=at(16)),
         E("Tick", EAGER), E("Tick", CAPTURE), E("Tick", REPLAY),                                                        # -> at(19)
         E("DecodeLookup", EAGER, ("batch_spec_key_R", "plan_ensure_rows>Tick", "batch_scratch_gen>Tick"), first=[105, 106, 107, 108], past=at(19), n=8, draft_max=3),
         E("DecodeLookup", REPLAY, first=[109, 110, 111, 112], past=at(27), n=8, draft_max=3),
         E("Set", tokens=[113, 114, 115, 116], past=at(35)),
         E("Tick", CAPTURE), E("Tick", REPLAY),                                                                          # -> at(37)
         E("SetSampler", None, ("batch_sampling", "batch_spec_key_sampled"), topK=40, seed=3, ring=64),
         E("DecodeSampleLookup", CAPTURE, first=[117, 118, 119, 120], past=at(37), n=8, draft_max=3),
         E("DecodeSampleLookup", REPLAY, first=[121, 122, 123, 124], past=at(45), n=8, draft_max=3),
         E("ClearSampler", None, ("batch_sampling", "batch_spec_key_sampled", "batch_spec_key_R")),
         E("DecodeLookup", CAPTURE, first=[125, 126, 127, 128], past=at(53), n=8, draft_max=1), E("DecodeLookup", REPLAY, first=[129, 130, 131, 132], past=at(61), n=8, draft_max=1),
         E("CacheImage", pos=at(69))]
    return Script("batch.lookup_among_ticks", "batch", "small", 256, tuple(s), PODS, lookup_among_ticks.__doc__)


def batches_come_and_go(weights):
    """A second batch of 8 pods on the same model is created, ticked and freed between two ticks of the first."""
    V = VOCAB["small"]
    s = [E("Prompt", EAGER, prompts=_prompts(V, (5, 7, 6, 9))),
         E("Tick", EAGER), E("Tick", CAPTURE), E("Tick", REPLAY),
         D("OtherBatch", None, ("other_object_freed",), pods=8, prompts=_prompts(V, (6,) * 8, seed=20), ticks=3),
         E("Tick", REPLAY), E("Tick", REPLAY),
         E("CacheImage", pos=[5 + 5, 7 + 5, 6 + 5, 9 + 5])]
    return Script("batch.batches_come_and_go", "batch", "small", 256, tuple(s), PODS, batches_come_and_go.__doc__)


BUILDERS = (growing_prompts, resident_around_detours, sampler_reconfiguration, speculation_interleaved, more_than_4096_ids, longer_window_appears,
            ticks_around_feeds, sampler_on_off_on, fork_and_unfork, lookup_among_ticks, batches_come_and_go)
SCRIPTS = {b("f32").name: b for b in BUILDERS}
CASES = [(name, w) for name in SCRIPTS for w in WEIGHTS]
