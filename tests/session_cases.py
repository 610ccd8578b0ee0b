"""The trigger table and the scripts of the session tests (tests/session_ref.py runs them; no GPU needed to import).

TRIGGERS lists every place in csrc/plan.hip, plan.h, score.hip, abi.hip, comm.hip, common.h and graph_cache.h that re-allocates something or drops / re-keys a captured graph (found by
reading every call of the grow helper `grow(`, every `hipFree(`, every generation counter `*_gen` and every key struct of a CapturedGraph in those files; the last field of a row
names the identifiers of the source it answers for, and tests/test_session_cpu.py::test_the_table_names_what_the_source_has collects them from the source again: a counter, key
field or grown buffer no row names fails there, and so does a row that names one the source no longer has).  Each row says what a captured graph must do behind it:
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
WEIGHTS = ("f32", "q8", "f16", "q4")
# f16 schedules as fp32 over the widened image (Plan::md_wide, plan.hip sched_md) and block-int4 as block-int8 over the expanded one: the same tile-GEMM thresholds
# (193 rows fp32 / f16: split-K; 89 rows block-int8 / block-int4: the xs3 planes) and the same bit-identical row limits (gemv_rows_max: 8 rows fp32 / f16, 4 block-int8 / -int4)
LIKE_F32 = ("f32", "f16")
# shapes of the scripts that mlapi.SHAPES does not name: the 2-layer 7B layer shape of tests/test_gpu_f16_tiles.py, the smallest on which gemm_mfma_group hands a 193-row prompt to k_gemm_b9
SHAPES = {"7Blayer2": dict(vocab=2048, embd=4096, mult=256, heads=32, layers=2)}
VOCAB["7Blayer2"] = 2048

RECAPTURE, KEEP = "recapture", "keep"

# name -> (where, what fires it, what a captured graph must do behind it, scripts that fire it or the reason none does, the identifiers of the source it answers for: IDENTIFIERS below)
_ROWS = {
    "plan_ensure_rows": ("plan.hip plan_ensure_rows", "an Eval / Score / Verify / feed pass of more rows than the plan's scratch holds: every scratch buffer, the "
                         "s3 planes and tokens_dev move, scratch_gen grows (in every key: DecodeKey, TickKey, Spec::Key, BatchSpec::Key)", RECAPTURE,
                         ("solo.growing_prompts", "solo.resident_around_detours", "solo.speculation_interleaved", "batch.ticks_around_feeds", "batch.lookup_among_ticks", "solo.tiles_and_stream")),
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
                        ("solo.resident_around_detours", "solo.switch_among_lookup_runs")),
    "score_dev": ("score.hip lh_llama_score", "a Score of more rows than score_dev holds: score_dev moves; no graph holds it", KEEP, ("solo.resident_around_detours",)),
    "verify_pass": ("plan.hip lh_llama_verify", "the speculative state of a plan is created beside live decode graphs (spec_ensure); nothing they hold moves", KEEP,
                    ("solo.resident_around_detours",)),
    "eval_cache": ("host/llamago.cpp llama_Eval (llamago_KeepDecodeGraph)", "the host mirror keeps the one-token ml graph between Evals and moves its position: an n-row "
                   "Eval between two one-token Evals must not leave the kept graph on the old scratch", RECAPTURE, ("solo.growing_prompts", "solo.tiles_and_stream")),
    "ensure_splitk": ("plan.hip ensure_splitk (grow)", "a split-K launch of more partial products than the context's buffer holds: splitk moves, splitk_gen "
                      "grows (the batch tick and both verify passes compare it; solo decode graphs hold no split-K buffer)", RECAPTURE,
                      ("solo.growing_prompts", "batch.ticks_around_feeds")),
    "ensure_xs3": ("plan.hip ensure_xs3", "block-int8 and block-int4, a prompt from 89 rows on (and an f16 prompt on k_gemm_b9_h): the context's bf16 planes move, splitk_gen grows", RECAPTURE,
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
                         RECAPTURE, ("solo.speculation_interleaved", "solo.switch_among_lookup_runs", "pair.draft_among_resident_runs")),
    "spec_trace_growth": ("plan.hip spec_ensure / batch_spec_ensure (trace)", "a lookup run of more passes than the trace buffer holds (4096): the buffer moves, the keys' trace "
                          "differs", RECAPTURE, "not covered: needs a lookup run of more than 4096 ids per call, which no script's window allows in a few seconds"),
    "batch_scratch_gen": ("plan.hip batch_tick_unchecked (TickKey::scratch_gen)", "a feed grows pod 0's scratch to FEED_PASS_ROWS, or a pod's own Eval (a feed of "
                          "LLAMAHIP_FEED_SOLO_MIN rows and more) grows that pod's: the sum of the pods' scratch_gen moves", RECAPTURE,
                          ("batch.ticks_around_feeds", "batch.lookup_among_ticks")),
    "feed_dev": ("plan.hip batch_feed (feed_dev, feed_part)", "a feed whose tables need more bytes than feed_dev holds; only the feed's own eager passes read it", KEEP,
                 ("batch.ticks_around_feeds",)),
    "batch_sampling": ("plan.hip batch_tick_unchecked (TickKey::sampling)", "lh_batch_set_sampler on or off: the tick ends in another kernel", RECAPTURE,
                       ("batch.sampler_on_off_on", "batch.lookup_among_ticks", "batch.switch_among_ticks")),
    "batch_ring_growth": ("plan.hip lh_batch_set_sampler", "a ring larger than ring_cap: ring_dev moves, Batch::smp_gen grows (TickKey::smp_gen)", RECAPTURE, ("batch.sampler_on_off_on", "batch.switch_among_ticks")),
    "batch_sampler_variant": ("plan.hip lh_batch_set_sampler", "topK crosses 64: Batch::smp_gen grows (TickKey::smp_gen)", RECAPTURE, ("batch.sampler_on_off_on",)),
    "batch_ring_smaller": ("plan.hip lh_batch_set_sampler", "a ring smaller than ring_cap, same variant: every ring re-initialised in place with the new size", KEEP,
                           ("batch.sampler_on_off_on",)),
    "env_sample_per_pod": ("plan.hip batch_tick_unchecked (TickKey::per_pod)", "LLAMAHIP_SAMPLE_PER_POD changes between two ticks", RECAPTURE, ("batch.sampler_on_off_on",)),
    "batch_shared": ("plan.hip batch_tick_unchecked (TickKey::shared)", "the block table goes from no block to some block (a fork) or back (LLAMAHIP_SHARE_ROW_ATTN)", RECAPTURE,
                     ("batch.fork_and_unfork", "batch.switch_among_ticks")),
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
    "comm_host_buffers": ("comm.hip grow (send_host, recv_host)", "the pinned host buffers of a communicator's exchange grow; copies from them are enqueued outside every capture", KEEP,
                          "not covered: needs ranks"),
    # ---- the switches that choose a kernel, and the context-owned weight images ----
    "f16_stream_switch": ("abi.hip lh_ctx_set_f16_stream / plan.hip f16_stream_key, f16_stream_sync", "the switch changes on a context of f16 plans: f16_stream_gen grows, the key field "
                          "of the tick and of both lookup passes changes (TickKey::f16_stream, Spec::Key::f16_stream, BatchSpec::Key::f16_stream) and f16_stream_sync clears their warm "
                          "bits - one EAGER pass (the kernels the new value chooses set their LDS attribute there), then a capture.  A solo lookup pass takes the Rows route and holds no "
                          "stream launch; its key carries the field all the same, so it re-captures too", RECAPTURE, ("solo.switch_among_lookup_runs", "batch.switch_among_ticks")),
    "q4_stream_switch": ("abi.hip lh_ctx_set_q4_stream / plan.hip f16_stream_key, f16_stream_sync", "the same for lh_ctx_set_q4_stream on a context of block-int4 plans: q4_stream_gen, "
                         "carried in the same key fields", RECAPTURE, ("solo.switch_among_lookup_runs", "batch.switch_among_ticks")),
    "stream_switch_other_type": ("plan.hip f16_stream_key", "lh_ctx_set_q4_stream on f16 plans / lh_ctx_set_f16_stream on block-int4 plans: the counter of the OTHER switch grows, "
                                 "f16_stream_key reads only the switch of the plan's own weight type (0 for fp32 and block-int8 plans)", KEEP,
                                 ("solo.switch_among_lookup_runs", "batch.switch_among_ticks")),
    "stream_switch_same_value": ("abi.hip lh_ctx_set_f16_stream / lh_ctx_set_q4_stream", "the switch set to the value it has: no counter moves", KEEP, ("solo.switch_among_lookup_runs",)),
    "stream_switch_decode_graphs": ("graph_cache.h DecodeKey", "the stream switch changes beside the five decode slots of a solo plan: a decode step is one row (the Step route), no stream "
                                    "launch stands in it and DecodeKey has no such field", KEEP, ("solo.tiles_and_stream",)),
    "f16_tiles_switch": ("abi.hip lh_ctx_set_f16_tiles", "the tile switch changes: no key field - only k_gemm_b9 launches read it (more than 128 rows), which no capture contains", KEEP,
                         ("solo.tiles_and_stream",)),
    "wide_image": ("plan.hip wide_image (lh_ctx::wide)", "another plan of the same size is made on the lh_ctx (a context's resident plan beside llama_Eval's, the draft of a pair of one "
                   "shape): it is handed the images that exist; an image never moves and is freed with the context", KEEP, ("pair.draft_among_resident_runs", "pair.replace_draft")),
    # ---- a draft pair: two plans, one lh_ctx, the target's Spec state ----
    "draft_plan_ensure_rows": ("plan.hip spec_decode_draft (plan_ensure_rows(p, R))", "a draft run of more rows per pass than the TARGET's resident scratch holds: as plan_ensure_rows, on "
                               "the target's plan - its decode graphs and its lookup pass re-capture", RECAPTURE, ("pair.draft_among_resident_runs",)),
    "draft_out_tokens": ("plan.hip spec_decode_draft (ensure_out_tokens(d, SPEC_ROWS_MAX))", "the DRAFT plan's output list is made by its first draft run.  Not the verdict of "
                         "ensure_out_tokens: the list's floor is 4096 ids, so this call allocates only on a plan whose list does not exist yet - a plan that has never run a resident call "
                         "and has no decode graph that could hold an older list; the target's graphs hold nothing of the draft's", KEEP, ("pair.draft_among_resident_runs", "pair.replace_draft")),
    "draft_shares_spec": ("plan.hip spec_decode_draft (spec_set, Spec::smp = false) / draft_enqueue_pass", "a draft run between lookup runs of the target: it runs eagerly on the target's "
                          "Spec state - row table, pending tokens, output list, smp - and touches no field of Spec::Key by itself, so the captured pass behind it replays (after a sampled "
                          "run as well: the next run sets smp itself)", KEEP, ("pair.draft_among_resident_runs", "pair.replace_draft")),
    "replace_draft": ("host/llamago.cpp llamago_DraftPairReplaceDraft (plan_destroy of the draft's plans)", "the draft context and its plans are freed beside the target's live graphs, "
                      "a fresh draft is made on the same lh_ctx (and is handed the same images when its size is the same)", KEEP, ("pair.replace_draft",)),
    "pair_shared_buffers": ("plan.hip ensure_splitk / ensure_xs3 on the pair's one lh_ctx", "a long prompt on the DRAFT side grows the split-K buffer (the xs3 planes) the target's plans "
                            "use too: splitk_gen grows, as ensure_splitk / ensure_xs3 - the target's lookup pass compares it and re-captures, its decode graphs hold no such buffer", RECAPTURE,
                            ("pair.draft_among_resident_runs",)),
}
# what each row answers for in the source: generation counters as they are spelt, key fields as Struct::field (Spec::Key / BatchSpec::Key for the two structs named Key), the buffers of
# grow( calls as the call spells them
IDENTIFIERS = {
    "plan_ensure_rows": ("scratch_gen", "DecodeKey::scratch_gen", "Spec::Key::scratch_gen", "BatchSpec::Key::scratch_gen"),
    "ensure_out_tokens": ("out_gen", "DecodeKey::out_gen", "p->out_tokens_dev", "Spec::Key::out"),
    "solo_sampler_variant": ("smp_gen", "DecodeKey::smp_gen", "Spec::Key::smp_small"),
    "solo_ring_growth": ("p->ring_dev", "Spec::Key::ring"),
    "plan_embeddings": ("p->emb",),
    "ensure_splitk": ("splitk_gen", "ctx->splitk", "TickKey::splitk_gen", "Spec::Key::splitk_gen", "BatchSpec::Key::splitk_gen"),
    "spec_key_R": ("Spec::Key::R",),
    "spec_key_lookup": ("Spec::Key::lp", "s->corpus"),
    "spec_key_sampled": ("Spec::Key::smp",),
    "spec_trace_growth": ("s->trace", "Spec::Key::trace", "Spec::Key::trace_cap", "BatchSpec::Key::trace", "BatchSpec::Key::trace_cap"),
    "batch_scratch_gen": ("TickKey::scratch_gen",),
    "feed_dev": ("b->feed_dev",),
    "batch_sampling": ("TickKey::sampling",),
    "batch_ring_growth": ("b->ring_dev", "TickKey::smp_gen"),
    "env_sample_per_pod": ("TickKey::per_pod",),
    "batch_shared": ("TickKey::shared",),
    "env_share_qb": ("TickKey::share_qb",),
    "batch_spec_key_R": ("BatchSpec::Key::R", "BatchSpec::Key::lp"),
    "batch_spec_key_sampled": ("BatchSpec::Key::smp", "BatchSpec::Key::small_k", "BatchSpec::Key::ss", "BatchSpec::Key::ring", "BatchSpec::Key::ring_cap"),
    "batch_x_in_out": ("TickKey::x_in", "TickKey::x_out"),
    "comm_host_buffers": ("cm->send_host", "cm->recv_host"),
    "f16_stream_switch": ("f16_stream_gen", "TickKey::f16_stream", "Spec::Key::f16_stream", "BatchSpec::Key::f16_stream"),
    "q4_stream_switch": ("q4_stream_gen",),
}
TRIGGERS = {name: row + (IDENTIFIERS.get(name, ()),) for name, row in _ROWS.items()}
assert set(IDENTIFIERS) <= set(_ROWS)


def E(call, trace=None, fires=(), rx=KERNEL_RE, **kw):
    extra = {k: kw.pop(k) for k in ("env", "equals", "twin", "note", "want", "wantnot") if k in kw}
    return Step(call, kw, ESSENTIAL, trace, tuple(fires), rx, **extra)


def D(call, trace=None, fires=(), rx=KERNEL_RE, **kw):
    extra = {k: kw.pop(k) for k in ("env", "equals", "twin", "note", "want", "wantnot") if k in kw}
    return Step(call, kw, DETOUR, trace, tuple(fires), rx, **extra)


# ---- solo ------------------------------------------------------------------------------------------------------------------------------------------------
def growing_prompts(weights):
    """One-token Evals (the G_STEP graph through the host mirror's kept ml graph) around prompts of 20, 70 and 200 (block-int8 and block-int4: 100) rows, each a detour at a
    rewound position: every growth moves the scratch, the last one crosses into the tile GEMM (fp32 and f16 193+: split-K; block-int8 and block-int4 89+: the xs3 planes)."""
    V = VOCAB["small"]
    big = 200 if weights in LIKE_F32 else 100   # (plan.hip: the fp32 tile GEMM with split-K from 193 rows - f16 runs it over the widened image; k_gemm_q8b3 over xs3 planes from Q8B_PROMPT_ROWS + 1 = 89 - block-int4 over the expanded image)
    last = ("plan_ensure_rows", "ensure_staging", "prefill_scratch") + (("ensure_splitk",) if weights in LIKE_F32 else ("ensure_xs3",))
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
    """Lookup-draft runs of R = 4, a plain resident run, R = 8 (block-int8 and block-int4: 2, their limit is 4 rows) with another n-gram range, a corpus, a sampled lookup run,
    R = 4 again (the prompt goes in as a Score of 12 rows on the resident plan, so that neither R = 8 nor the sampled run's 10-row prompt grows its scratch: the
    captures behind them are the pass key's alone), and a 70-row Score detour between two R = 4 runs (scratch_gen moves under the pass graph; an Eval would not do: it runs on
    the context's other plan, see resident_around_detours)."""
    V = VOCAB["small"]
    k2 = 7 if weights in LIKE_F32 else 1   # (plan.hip gemv_rows_max: 8 rows fp32 and f16, GEMV_ROWS_MAX_Q8 = 4 block-int8 and block-int4; R = 4 is taken by the first runs)
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
    big = ("plan_ensure_rows", "batch_scratch_gen") + (("ensure_splitk",) if weights in LIKE_F32 else ("ensure_xs3",))
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


# ---- the switches that choose a kernel (f16 and block-int4 only: on another weight type they do nothing, tests/test_gpu_f16_stream.py holds that) ----------------
def _switches(weights):
    """(the stream switch of the weight type, the other type's, the trigger row of the first, a route-trace pattern of the kernels the first one chooses)"""
    if weights == "f16":
        return "lh:f16_stream", "lh:q4_stream", "f16_stream_switch", r"^k_stream_(mm2|dma)_h<"
    return "lh:q4_stream", "lh:f16_stream", "q4_stream_switch", r"^k_stream_q4b<"


def switch_among_lookup_runs(weights):
    """Lookup runs of R = 4 with the stream switch off, on (one eager pass, a capture, replays), under it a 33-row Score and a 70-row Eval detour (the launches the switch
    chooses: k_stream_*_h / k_stream_q4b reading halves / nibbles, every other launch site filling its own image slot) and a sampled lookup run, then off, on, on again (the
    value it has: nothing moves) and the OTHER weight type's switch (its counter is not in this plan's key).  The prompt goes in as a Score of 40 rows on the resident plan, so
    that the 33-row Score grows nothing, and both detours run once with the switch off first: every capture behind a toggle is the key field's alone.  A solo lookup pass is a Rows-route pass and holds no stream launch; the
    key carries the switch all the same (the row says so), and the poisoned images hold every pass of it to the twins."""
    V = VOCAB["small"]
    own, other, row, chosen = _switches(weights)
    run = lambda trace, first, past, fires=(), **kw: E("DecodeLookup", trace, fires, rx=ROWS_RE, first=first, past=past, n=16, draft_max=3, **kw)   # noqa: E731
    s = [E("Score", EAGER, tokens=toks(40, 1, V), past=0),
         # the two detours once with the switch off: every grow-only buffer of the context (the split-K buffer, whose generation the pass key holds) is then at the size
         # these row counts need, and the same detours under the switch - "the schedule, every kernel shape and every sum are the twin's" (include/llamahip.h) - grow nothing
         D("Score", EAGER, tokens=toks(33, 2, V), past=40, wantnot=(chosen,)), D("Eval", EAGER, tokens=toks(70, 3, V), past=40, wantnot=(chosen,)),
         run(EAGER, 31, 40), run(REPLAY, 32, 56),
         run(EAGER, 33, 72, (row,), env=((own, "1"),)), run(REPLAY, 34, 88),
         D("Score", EAGER, tokens=toks(33, 2, V), past=104, want=(chosen,)),
         run(REPLAY, 35, 104),
         D("Eval", EAGER, ("other_plan_rows",), tokens=toks(70, 3, V), past=120, want=(chosen,)),
         run(REPLAY, 36, 120),
         E("SampleDecodeLookup", CAPTURE, ("spec_key_sampled",), rx=ROWS_RE, prompt=toks(10, 4, V), n=16, draft_max=3, ring=64, topK=40, seed=7, want=(chosen,)),
         run(CAPTURE, 37, 25, ("spec_key_sampled",)), run(REPLAY, 38, 41),
         run(EAGER, 39, 57, (row,), env=((own, None),)), run(REPLAY, 40, 73),
         run(EAGER, 41, 89, (row,), env=((own, "1"),)), run(REPLAY, 42, 105),
         run(REPLAY, 43, 121, ("stream_switch_same_value",), env=((own, "1"),)),
         run(REPLAY, 44, 137, ("stream_switch_other_type",), env=((other, "1"),)), run(REPLAY, 45, 153),
         E("CacheImage", pos=169)]
    return Script("solo.switch_among_lookup_runs", "solo", "small", 256, tuple(s), doc=switch_among_lookup_runs.__doc__)


switch_among_lookup_runs.weights = ("f16", "q4")


def tiles_and_stream(weights):
    """f16 on the 2-layer 7B layer shape (the smallest on which a 193-row prompt takes k_gemm_b9): one-token Evals (G_STEP) and the resident loop around prompts of 33 rows (the
    stream kernels) and 193 rows (the tile GEMM), both detours at a rewound position, under each of the four combinations of lh_ctx_set_f16_stream and lh_ctx_set_f16_tiles.
    Neither switch is in a DecodeKey: behind every toggle the one-token Eval and the resident loop replay.  With the tile switch on the 193-row prompt must launch k_gemm_b9_h,
    with the stream switch on the 33-row prompt k_stream_*_h; whichever is on, every launch that still reads fp32 widens its own matrices (the poisoned image holds it to that).
    The first 193-row prompt under the tile switch grows the context's xs3 planes (ensure_xs3: splitk_gen), which no graph of a solo decode step holds."""
    V = VOCAB["7Blayer2"]
    H, T = "lh:f16_stream", "lh:f16_tiles"
    one = lambda trace, tok, past, fires=(), **kw: E("Eval", trace, fires, rx=DECODE_RE, tokens=[tok], past=past, **kw)   # noqa: E731
    dec = lambda trace, first, past: E("Decode", trace, rx=DECODE_RE, first=first, past=past, n=6)   # noqa: E731
    s = [E("Eval", EAGER, tokens=toks(3, 1, V), past=0), one(CAPTURE, 11, 3), one(REPLAY, 12, 4),
         dec(CAPTURE, 21, 5), dec(REPLAY, 22, 11),                                                                         # -> 17
         D("Eval", EAGER, ("plan_ensure_rows", "eval_cache"), tokens=toks(33, 2, V), past=17, wantnot=(r"^k_stream_\w+_h<",)),
         D("Eval", EAGER, ("plan_ensure_rows",), tokens=toks(193, 3, V), past=17, want=(r"^k_gemm_b9<",), wantnot=(r"^k_gemm_b9_h<", r"^k_stream_\w+_h<")),
         one(CAPTURE, 13, 17), one(REPLAY, 14, 18), dec(REPLAY, 23, 19)]                                                   # -> 25
    past, tok = 25, 15
    for k, (h, t) in enumerate(((1, 0), (1, 1), (0, 1), (0, 0))):
        fires = ("stream_switch_decode_graphs",) if k in (0, 2) else ("f16_tiles_switch",)   # (one switch moves per round: stream on, tiles on, stream off, tiles off)
        s += [one(REPLAY, tok, past, fires, env=((H, "1" if h else None), (T, "1" if t else None))), dec(REPLAY, 24 + k, past + 1),
              D("Eval", EAGER, tokens=toks(33, 4 + k, V), past=past + 7, want=(r"^k_stream_(mm2|dma)_h<",) if h else (), wantnot=() if h else (r"^k_stream_\w+_h<",)),
              D("Eval", EAGER, tokens=toks(193, 8 + k, V), past=past + 7, want=(r"^k_gemm_b9_h<",) if t else (r"^k_gemm_b9<",), wantnot=(r"^k_gemm_b9<",) if t else (r"^k_gemm_b9_h<",)),
              one(REPLAY, tok + 1, past + 7), dec(REPLAY, 34 + k, past + 8)]
        past, tok = past + 14, tok + 2
    s.append(E("CacheImage", pos=past))
    assert past + 193 <= 384
    return Script("solo.tiles_and_stream", "solo", "7Blayer2", 384, tuple(s), doc=tiles_and_stream.__doc__)


tiles_and_stream.weights = ("f16",)


def switch_among_ticks(weights):
    """Four pods, pod 0 behind a prompt of 260 keys (two full 128-key chunks, for the fork): ticks, the stream switch on, ticks; a 24-row feed and a 3 x 60-row feed under each
    value (the launches the switch chooses); lookup passes of 4 pods x R = 16 rows with a toggle between two runs (the captured TICK notices it too); sampled ticks with a
    toggle; a fork with the switch toggled while the pods share; the other weight type's switch.  A tick of four pods is a Rows-route pass without a stream launch: its key
    carries the switch all the same."""
    V = VOCAB["small"]
    own, other, row, chosen = _switches(weights)
    pos = [260, 7, 6, 9]
    s = [E("Feed", EAGER, tokens=[toks(260, 1, V), toks(7, 2, V), toks(6, 3, V), toks(9, 4, V)], past=[0, 0, 0, 0]),
         E("Set", tokens=[71, 72, 73, 74], past=list(pos))]

    def ticks(*traces, fires=(), **kw):
        for i, t in enumerate(traces):
            s.append(E("Tick", t, fires if i == 0 else (), **(kw if i == 0 else {})))
            pos[:] = [p + 1 for p in pos]

    def feed(lens, seed, fires=(), **kw):
        s.append(E("Feed", EAGER, fires, tokens=[toks(n, seed + i, V) if n else [] for i, n in enumerate(lens)], past=[p if n else 0 for p, n in zip(pos, lens)], **kw))
        pos[:] = [p + n for p, n in zip(pos, lens)]

    def lookup(trace, first, fires=(), **kw):
        s.append(E("DecodeLookup", trace, fires, first=[first + i for i in range(PODS)], past=list(pos), n=8, draft_max=3, **kw))
        pos[:] = [p + 8 for p in pos]

    # (the first Feed's batched pass has grown pod 0's scratch to the 64 rows of a feed pass.  Whether a later pass grows the context's split-K buffer depends on the
    # kernels' split counts; the script does not lean on it: the feeds under the first value stand in front of a toggle, whose ticks run eagerly and capture in any
    # case, and the same feeds under the second value find every grow-only buffer at its size - the schedule, every kernel shape and split count are the same under
    # both values - so the captured tick behind them must replay.)
    ticks(EAGER, CAPTURE, REPLAY)
    ticks(EAGER, CAPTURE, REPLAY, fires=(row,), env=((own, "1"),))
    feed((0, 24, 0, 0), 10, want=(chosen,))
    feed((0, 60, 60, 60), 20)
    ticks(EAGER, CAPTURE, REPLAY, fires=(row,), env=((own, None),))
    feed((0, 24, 0, 0), 30, wantnot=(chosen,))
    ticks(REPLAY)
    feed((0, 60, 60, 60), 40)
    ticks(REPLAY)
    lookup(EAGER, 91)
    lookup(REPLAY, 95)
    lookup(EAGER, 99, (row, row + ">Tick"), env=((own, "1"),), want=(chosen,))
    lookup(REPLAY, 103)
    s.append(E("Set", tokens=[111, 112, 113, 114], past=list(pos)))
    ticks(EAGER, CAPTURE, REPLAY)
    s.append(E("SetSampler", None, ("batch_sampling", "batch_ring_growth"), topK=40, seed=5, ring=64))
    ticks(CAPTURE, REPLAY)
    ticks(EAGER, CAPTURE, REPLAY, fires=(row,), env=((own, None),))
    s.append(E("ClearSampler", None, ("batch_sampling",)))
    ticks(CAPTURE, REPLAY)
    s.append(E("Fork", src=0, dst=[1], n_pos=pos[0]))
    pos[1] = pos[0]
    s.append(E("Set", tokens=[121, 122, 123, 124], past=list(pos)))
    ticks(CAPTURE, REPLAY, fires=("batch_shared",))
    ticks(EAGER, CAPTURE, REPLAY, fires=(row,), env=((own, "1"),))
    ticks(REPLAY, REPLAY, fires=("stream_switch_other_type",), env=((other, "1"),))
    s.append(E("CacheImage", pos=list(pos)))
    assert max(pos) <= 384
    return Script("batch.switch_among_ticks", "batch", "small", 384, tuple(s), PODS, switch_among_ticks.__doc__)


switch_among_ticks.weights = ("f16", "q4")


# ---- a draft pair: target and draft on one lh_ctx (session_ref.PAIRS: f32 target / block-int8 draft, f16 / f16 of the same shape, block-int4 / f32) --------
def _pair_ks(weights):
    """draft_len of the first and of the wider draft runs: R = 4 then 8 for an fp32 / f16 target, 2 then 4 for a block-int4 one (gemv_rows_max of the TARGET's weight type)"""
    return (3, 7) if weights in LIKE_F32 else (1, 3)


def draft_among_resident_runs(weights):
    """A prompt on both sides; the target's resident loop; the draft's plan appears beside it (an f16 draft of the target's shape is handed the target's images); DecodeDraft
    (the target's resident scratch grows to R rows under its decode graphs, the draft's output list is made), the target's Decode, DecodeDraft again (nothing moves); a sampled
    lookup run of the target as a detour in front of a draft run (the draft run must not inherit its smp); the target's DecodeLookup, a DecodeDraft of a wider draft_len (the
    scratch grows under the captured pass), DecodeLookup again; a DecodeDraft that moves nothing between two lookup runs; a 200-row (block-int8 draft: 100-row) detour on the
    DRAFT side, which grows the split-K buffer / the xs3 planes of the lh_ctx both sides share (the target's pass compares splitk_gen); the draft's own resident loop as a
    detour at a rewound position; the cache images of both sides.  Draft runs are eager, always.  The draft side is kept at the target's position by Evals of fixed tokens:
    what the draft proposes changes the pass lists, never the ids."""
    from session_ref import PAIRS
    V = VOCAB["small"]
    k1, k2 = _pair_ks(weights)
    big = 100 if PAIRS[weights][0] == "q8" else 200
    s, t, d, cap = [], [0], [0], [1]   # the steps, the positions of the two sides, the rows of the target's resident scratch
    WARM, warmed = 48, []

    def tdec(trace, first, fires=()):
        s.append(E("target.Decode", trace, fires, rx=DECODE_RE, first=first, past=t[0], n=6))
        t[0] += 6

    def dfill(seed, fires=(), role=E):
        """the draft side brought to the target's position"""
        if t[0] > d[0]:
            assert t[0] - d[0] <= WARM or not warmed, (t, d)   # (behind the warm-up pass no fill may be the largest pass so far: see WARM)
            s.append(role("draft.Eval", EAGER, fires, tokens=toks(t[0] - d[0], seed, V), past=d[0]))
            d[0] = t[0]

    def draft(first, k, extra=()):
        grows = k + 1 > cap[0]
        cap[0] = max(cap[0], k + 1)
        s.append(E("DecodeDraft", EAGER, (("draft_plan_ensure_rows",) if grows else ()) + tuple(extra), rx=ROWS_RE, first=first, past=t[0], n=12, draft_len=k))
        t[0] += 12
        d[0] = t[0]
        return grows

    def tlook(trace, first, k, fires=()):
        cap[0] = max(cap[0], k + 1)
        s.append(E("target.DecodeLookup", trace, fires, rx=ROWS_RE, first=first, past=t[0], n=12, draft_max=k))
        t[0] += 12

    s.append(E("target.Eval", EAGER, tokens=toks(6, 1, V), past=0))
    t[0] = 6
    tdec(CAPTURE, 21)
    tdec(REPLAY, 22)
    # The draft's plan appears - as a detour of WARM rows, more than any fill behind the first captured lookup pass has.  The split-K buffer belongs to the lh_ctx
    # both sides share and the target's pass key holds its generation; a stream / planes pass needs S x rows x M floats of it with S fixed by the shape (plan.hip
    # gemm_stream_split, gemm_q8b_split), so it grows exactly when a pass has more rows than any before it.  With this pass in front, the fills that keep the draft at
    # the target's position grow nothing, and the one growth the script means - the long prompt on the draft side - is the only one under the captured pass.
    s.append(D("draft.Eval", EAGER, ("wide_image",), tokens=toks(WARM, 14, V), past=0))
    warmed.append(True)
    tdec(REPLAY, 23)
    dfill(3)
    draft(24, k1, ("draft_out_tokens",))
    tdec(CAPTURE, 25)
    tdec(REPLAY, 26)
    dfill(4)
    draft(27, k1)
    tdec(REPLAY, 28)
    # a sampled lookup run as a detour: it rewrites rows [0, 2 + 8) of the target's cache, the Eval behind it puts the script's tokens back (two prompt rows, R = 2: it grows nothing on any target)
    s.append(D("target.SampleDecodeLookup", EAGER, rx=ROWS_RE, prompt=toks(2, 5, V), n=8, draft_max=1, ring=64, topK=40, seed=7))
    s.append(E("target.Eval", EAGER, tokens=toks(t[0], 6, V), past=0))
    dfill(7)
    draft(29, k1, ("draft_shares_spec",))
    tdec(REPLAY, 30)
    dfill(8)
    tlook(EAGER, 31, k1)
    tlook(REPLAY, 32, k1)
    dfill(9)
    assert draft(33, k2, ("draft_shares_spec",))
    tlook(CAPTURE, 34, k1)
    tlook(REPLAY, 35, k1)
    tdec(CAPTURE, 36)
    tdec(REPLAY, 37)
    dfill(10)
    draft(38, k1, ("draft_shares_spec",))
    tlook(REPLAY, 39, k1)
    tdec(REPLAY, 40)
    assert d[0] + big <= 384, d
    s.append(D("draft.Eval", EAGER, ("pair_shared_buffers>target.DecodeLookup",), tokens=toks(big, 11, V), past=d[0]))
    dfill(12)
    draft(41, k1)
    tlook(CAPTURE, 42, k1)
    tlook(REPLAY, 43, k1)
    tdec(REPLAY, 44)
    s.append(D("draft.Decode", CAPTURE, rx=DECODE_RE, first=45, past=d[0], n=8))
    s.append(D("draft.Decode", REPLAY, rx=DECODE_RE, first=46, past=d[0] + 8, n=8))
    dfill(13)
    draft(47, k1)
    tdec(REPLAY, 48)
    # a draft run between two SAMPLED lookup runs of the target (essential: they start again from a 4-row prompt at position 0, within the scratch).  The first
    # captures the sampled pass (Spec::Key::smp and the output offset), the draft run sets smp = false on the same Spec and runs eagerly, the second sets smp itself:
    # its passes must replay, and its ids repeat the first run's byte for byte
    smp = dict(prompt=toks(4, 15, V), n=8, draft_max=k1, ring=64, topK=40, seed=7)
    s.append(E("target.SampleDecodeLookup", CAPTURE, ("spec_key_sampled",), rx=ROWS_RE, **smp))
    first_sampled = len(s) - 1
    s.append(E("DecodeDraft", EAGER, ("draft_shares_spec",), rx=ROWS_RE, first=49, past=12, n=12, draft_len=k1))
    s.append(E("target.SampleDecodeLookup", REPLAY, rx=ROWS_RE, equals=first_sampled, **smp))
    s.append(E("CacheImage", pos=12, draft_pos=24))
    assert t[0] <= 384 and d[0] + 16 <= 384, (t, d)
    return Script("pair.draft_among_resident_runs", "pair", "small", 384, tuple(s), doc=draft_among_resident_runs.__doc__)


draft_among_resident_runs.weights = ("f32", "f16", "q4")


def replace_draft(weights):
    """A draft run behind the prompts, resident and lookup runs of the target (its prompt a 12-row Score on the resident plan: no later pass grows the scratch), then
    ReplaceDraft - the draft context and its plans freed beside the target's live graphs, a fresh draft over another model on the same lh_ctx - and the target's runs
    again (replay).  The new draft is re-prompted with two Evals of 4 rows (the Rows route of every weight type: GEMV launches, which size no buffer of the context -
    a longer prompt could grow the split-K buffer both sides share, which the target's pass compares, and the script would then lean on the kernels' split counts);
    a draft run with it from position 8, where both sides have rows, makes its output list; the target's runs go on from there (replay).  Detours, which the fresh
    twin never runs: the OLD draft's own resident loop just in front of ReplaceDraft (its decode graphs and its output list are what ReplaceDraft frees beside the
    target's), and an 8-row Score of the target at a rewound position on either side of the new draft's first run (it runs on the target's resident plan, within the
    12 rows the prompt sized: nothing grows, the graphs behind it replay)."""
    V = VOCAB["small"]
    k1, _ = _pair_ks(weights)
    look = lambda trace, first, past, fires=(): E("target.DecodeLookup", trace, fires, rx=ROWS_RE, first=first, past=past, n=12, draft_max=k1)   # noqa: E731
    dec = lambda trace, first, past: E("target.Decode", trace, rx=DECODE_RE, first=first, past=past, n=8)   # noqa: E731
    s = [E("target.Score", EAGER, tokens=toks(12, 1, V), past=0), E("draft.Eval", EAGER, tokens=toks(12, 1, V), past=0),
         E("DecodeDraft", EAGER, rx=ROWS_RE, first=20, past=12, n=12, draft_len=k1),                                          # -> 24
         dec(CAPTURE, 21, 24), dec(REPLAY, 22, 32),                                                                          # -> 40
         look(EAGER, 23, 40), look(REPLAY, 24, 52),                                                                          # -> 64
         D("draft.Decode", CAPTURE, rx=DECODE_RE, first=41, past=24, n=8), D("draft.Decode", REPLAY, rx=DECODE_RE, first=42, past=32, n=8),
         E("ReplaceDraft", None, ("replace_draft",)),
         dec(REPLAY, 25, 64), look(REPLAY, 26, 72),                                                                          # -> 84
         E("draft.Eval", EAGER, ("wide_image",), tokens=toks(4, 3, V), past=0),
         dec(REPLAY, 27, 84),                                                                                                # -> 92
         D("target.Score", EAGER, tokens=toks(8, 5, V), past=92),
         dec(REPLAY, 43, 92),                                                                                                # -> 100
         E("draft.Eval", EAGER, tokens=toks(4, 4, V), past=4),
         E("DecodeDraft", EAGER, ("draft_out_tokens", "draft_shares_spec"), rx=ROWS_RE, first=28, past=8, n=12, draft_len=k1),   # -> 20, both sides
         look(REPLAY, 29, 20),                                                                                               # -> 32
         D("target.Score", EAGER, tokens=toks(8, 6, V), past=32),
         dec(REPLAY, 30, 32),                                                                                                # -> 40
         E("CacheImage", pos=40, draft_pos=20)]
    return Script("pair.replace_draft", "pair", "small", 256, tuple(s), doc=replace_draft.__doc__)


replace_draft.weights = ("f32", "f16", "q4")

BUILDERS = (growing_prompts, resident_around_detours, sampler_reconfiguration, speculation_interleaved, more_than_4096_ids, longer_window_appears,
            ticks_around_feeds, sampler_on_off_on, fork_and_unfork, lookup_among_ticks, batches_come_and_go,
            switch_among_lookup_runs, tiles_and_stream, switch_among_ticks, draft_among_resident_runs, replace_draft)
SCRIPTS = {b(getattr(b, "weights", WEIGHTS)[0]).name: b for b in BUILDERS}
# every script runs for every weight type, except: the switch scripts (f16 and block-int4 only: the switches do nothing on another type, which the f16 / q4 stream tests hold),
# the tile script (f16: there is no tile switch for another type) and the pair scripts (the three pairs of session_ref.PAIRS, named by the target's type)
CASES = [(name, w) for name, b in SCRIPTS.items() for w in getattr(b, "weights", WEIGHTS)]
