/* include/llamago_ext.h — the llamago_* exports of the host libraries: entry points with NO counterpart in the reference
 * (gotzmann/llama.go), needed by harnesses (tests/, bench.py), by the device-resident loops and by the multi-GPU / multi-pod
 * paths.  include/llamago.h stays the mirror of the reference's own names; everything else a host library exports is declared
 * HERE, and tests/test_abi.py diffs `nm -D` of both libraries against the two headers in both directions, so that the hand-written
 * ctypes / cgo bindings cannot drift from the C++ definitions unnoticed (the product host includes this header: signatures are
 * compiler-checked).
 *
 *   [both]     exported by llama.go_amd/lib/libllamago.so AND by the checker library oracle/liboracle.so
 *   [product]  libllamago.so only (needs the MI355X backend)
 */
#ifndef LLAMAGO_EXT_H
#define LLAMAGO_EXT_H
#include "llamago.h"
#include "llamahip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- [both] harness helpers ------------------------------------------------------------------------------------------- */
/* Releases every tensor the calling thread's constructors made and no graph freed: stands where the reference forces
 * runtime.GC() after each Eval (llama.go:423). */
void llamago_CollectGarbage(void);
/* The graph llama.Eval builds for a model of shape hp, as numbers (needs no GPU): per tensor 11 int32 = op, ne[4], nb[4], src0, src1
 * (indices into the same list, leafs first then nodes in ml.GraphCompute's order, -1 = nil).  Returns the tensor count. */
int llamago_DescribeEvalGraph(const llama_hparams* hp, uint32_t ctxSize, uint32_t N, uint32_t pastCount, int32_t* out, uint32_t cap_tensors, uint32_t* n_leafs);
/* The decode part of llama_GreedyDecode's loop on its own: from the context's present state (the caller has evaluated everything up to position
 * `past`), n_steps times { llama.Eval of ONE token = one ml_GraphCompute = one lh_graph_compute; the host argmax of its logits row }, starting with
 * `token`; out_tokens[s] = the id step s produced.  The contract route bench.py's headline times.  No context swap: past + n_steps
 * must stay inside the window. */
int llamago_GreedyContinue(llama_context* lctx, llama_model* m, uint32_t token, uint32_t past, uint32_t n_steps, uint32_t* out_tokens);
/* The greedy pick of the generation loops on host logits (strict >, the lowest index wins ties; a NaN at index 0 wins, NaNs elsewhere are skipped -
 * what `if x[i] > x[best] { best = i }` does).  Exported so that the product's vectorised form is tested against the checker's loop. */
uint32_t llamago_Argmax(const float* x, uint32_t n);
/* llama_SampleTopPTopK that also returns the kept candidates in rank order after the topP rescale (the reference's logitsID / probs
 * right before the random pick, llama.go:639-661). */
int llamago_SampleDebug(ml_context* ctx, const float* logits, uint32_t logitsCount, const uint32_t* lastNTokens, uint32_t lastNTokensSize, uint32_t topK, float topP,
                        float temp, float repeatPenalty, uint64_t seed, uint64_t draw, uint32_t* token, uint32_t* cand_ids, float* cand_probs, uint32_t* n_keep);
/* Block-int8 weight matrices (ML_TYPE_Q8_0, format ours: SURVEY §8a row 22).  Product: quantises every matrix in HBM and releases the
 * f32 copies; checker: replaces its weights by the dequantised values.  Before any context of the model exists. */
int llamago_QuantizeModelQ8(llama_model* m);

/* ---- [product] device plumbing ---------------------------------------------------------------------------------------- */
int llamago_DeviceCount(void);                       /* lh_device_count */
int llamago_HbmReadProbe(uint64_t bytes, uint32_t repeats, float* gbps);   /* lh_hbm_read_probe on the model context's device */
void llamago_SetStream(void* hip_stream);            /* HIP stream for contexts created from now on (NULL: a private one each) */
int llamago_Sync(llama_context* c);                  /* waits for the context's stream */
int llamago_TimeComputes(llama_context* c, int on);  /* lh_ctx_time_computes on the context llama_Eval computes in */
int llamago_ComputeStats(llama_context* c, uint64_t* calls, double* wall_us, double* device_us);   /* lh_ctx_compute_stats */
int llamago_LastGraphFused(ml_context* ctx);         /* 1 if the last ml_GraphCompute ran as the fused LLaMA plan */
int llamago_GraphComputeNoFusion(ml_context* ctx, ml_graph* g);   /* ml_GraphCompute node by node with the generic kernels (op-level parity) */
/* Test instrumentation: overwrites one fp32 tensor of the model ("layers.0.attention.wq.weight", "norm.weight", ...: llama_ModelTensor's names) in HBM with
 * `n` host floats, row-major as llama_ModelTensor / ml_TensorRead show it (lh_buf_upload).  Fails (non-zero, ml_LastError) on an unknown name, n different from
 * the tensor's element count, a block-int8 tensor, or a model with live contexts / batches / pipelines (their plans may hold derived copies). */
int llamago_SetModelTensor(llama_model* m, const char* name, const float* data, uint64_t n);
/* Test instrumentation: floats [off_floats, off_floats + n) of a context's KV cache (which: 0 = K, 1 = V) read to the host / overwritten from it, after
 * waiting for the context's stream.  The cache is [layer1 - layer0][ctxSize][embd] floats: slot = layer - layer0, then position, then channel, K and V
 * alike.  Fails (non-zero, ml_LastError) on a null argument, which outside 0 / 1, or a range outside the cache.  llamago_BatchCache*: pod `pod` of a batch
 * (declared with the batch below). */
int llamago_CacheRead(llama_context* c, int which, uint64_t off_floats, float* dst, uint64_t n);
int llamago_CacheWrite(llama_context* c, int which, uint64_t off_floats, const float* src, uint64_t n);
/* Test instrumentation: lh_ctx_poison_weight_images (llamahip.h) on the lh_ctx the context / the batch evaluates in - every fp32 image of f16 matrices and
 * every int8 image of block-int4 ones filled with 0xFF bytes behind the work already enqueued.  Returns the bytes filled (0 for an f32 or block-int8 model,
 * and before the first plan exists), -1 (ml_LastError) on a null argument or a HIP error.  llamago_BatchPoisonWeightImages is declared with the batch below. */
int64_t llamago_PoisonWeightImages(llama_context* c);
/* f16 weight matrices kept f16 in HBM (ML_TYPE_F16 = dtype 1 of llamahip.h; norm vectors and tok_embeddings stay f32).  Every Eval route of such a model
 * produces the bytes an f32 model holding the same values produces: one row and 2..8 rows on f16 forms of the decode stream kernels, every other row
 * count on the f32 kernels behind an exact widening pass.
 * llamago_LoadModelKeepF16: llama_LoadModel, except that a file whose weight matrices (seven per layer + output) are ALL f16 keeps them as halves
 *   (lh_tensor_register dtype 1, no f32 copy); any other file loads exactly as llama_LoadModel loads it.
 * llamago_NarrowModelF16 / llamago_WidenModelF16 (llamago_QuantizeModelQ8's shape; for synthetic models and the tests' f32 twin): the matrices through
 *   lh_buf_narrow_f16 (round to nearest even; *n_changed, optional, = elements whose value changed) / back through lh_buf_widen_f16 (exact), the old
 *   copies released.  Refused (non-zero, ml_LastError) while contexts, batches or pipelines of the model are alive, and on a block-int8 model.
 * llamago_ModelWeightType: 0 (f32) / 1 (f16) / 2 (block-int4) / 7 (block-int8).
 * On an f16 model llamago_SetModelTensor (of a matrix), llamago_QuantizeModelQ8 and llama_SaveModel refuse with a message that says so. */
llama_model* llamago_LoadModelKeepF16(const char* fileName, uint32_t ctxSize);
int llamago_NarrowModelF16(llama_model* m, uint64_t* n_changed);
int llamago_WidenModelF16(llama_model* m);
int llamago_ModelWeightType(const llama_model* m);
/* lh_ctx_set_f16_stream / lh_ctx_f16_stream (llamahip.h) on the lh_ctx the context / the batch evaluates in: with on != 0 the Evals of 2..128 rows of an
 * f16 model that take the stream kernels read the model's halves (k_stream_mm2_h / k_stream_dma_h) instead of an fp32 image widened in front of every
 * layer - the same bytes ("Native stream kernels").  Off by default (LLAMAHIP_F16_STREAM=1 turns it on for contexts created afterwards); without
 * effect on models of another weight type.  The setters return non-zero (ml_LastError) on a null argument; the getters 0 | 1.
 * llamago_BatchSetF16Stream / llamago_BatchF16Stream (declared with the batch below): the same for a batch's ticks, feeds and speculative passes. */
int llamago_SetF16Stream(llama_context* c, int on);
int llamago_F16Stream(llama_context* c);
/* lh_ctx_set_q4_stream / lh_ctx_q4_stream (llamahip.h) on the lh_ctx the context / the batch evaluates in: with on != 0 the Evals of a block-int4 model over
 * activation planes (5..64 rows of a tick, 5..88 of a prompt) read the model's nibbles (k_stream_q4b) instead of an int8 image expanded in front of every
 * layer - the same bytes ("Native stream kernel").  Off by default (LLAMAHIP_Q4_STREAM=1 turns it on for contexts created afterwards); without
 * effect on models of another weight type.  The setters return non-zero (ml_LastError) on a null argument; the getters 0 | 1.
 * llamago_BatchSetQ4Stream / llamago_BatchQ4Stream (declared with the batch below): the same for a batch's ticks, feeds and speculative passes. */
int llamago_SetQ4Stream(llama_context* c, int on);
int llamago_Q4Stream(llama_context* c);
/* lh_ctx_set_f16_tiles / lh_ctx_f16_tiles (llamahip.h) on the lh_ctx the context evaluates in: with on != 0 the Evals of more than 128 rows of an f16 model
 * run their k_gemm_b9 launches on the model's halves (k_gemm_b9_h: six bf16 products per tile pair instead of eight, no widening pass in front) - the same
 * bytes ("Native tile GEMM").  Off by default (LLAMAHIP_F16_TILES=1 turns it on for contexts created afterwards); without effect on models of
 * another weight type; independent of llamago_SetF16Stream.  The setter returns non-zero (ml_LastError) on a null argument; the getter 0 | 1. */
int llamago_SetF16Tiles(llama_context* c, int on);
int llamago_F16Tiles(llama_context* c);
/* Block-int4 weight matrices (ML_TYPE_Q4_0 = dtype 2 of llamahip.h: 20 bytes per 32 weights; norm vectors and tok_embeddings stay f32).  A 4-bit quant
 * q in [-8, 7] with block scale d IS a block-int8 weight with the same q and d, so every Eval route of such a model produces the bytes its expansion
 * produces: one row and 2..4 rows on 4-bit forms of the decode stream kernels, every other row count on the int8 kernels behind an exact expansion
 * pass.
 * llamago_QuantizeModelQ4 (llamago_QuantizeModelQ8's shape): every weight matrix of an f32 model through lh_buf_quantize_q4, the f32 copies released.
 * llamago_ExpandModelQ4: the matrices through lh_buf_expand_q4 - a block-int8 model with the same quants and scales.
 * Both are refused (non-zero, ml_LastError) while contexts, batches or pipelines of the model are alive, and on a model of another weight type.
 * llamago_ModelWeightType then returns 2 / 7.  On a block-int4 model llamago_SetModelTensor (of a matrix), llamago_QuantizeModelQ8,
 * llamago_NarrowModelF16 and llama_SaveModel refuse with a message that says so.
 * llamago_SaveModelQ4: a block-int4 model as a ggjt file of ftype 2 - the matrices as their 20-byte Q4_0 blocks {float d; uint8 qs[16]}, norm vectors
 *   and tok_embeddings f32.  llama_LoadModel refuses such a file as the reference does (llama.go:956-959).
 * llamago_LoadModelKeepQ4: llama_LoadModel, except that a file whose weight matrices (seven per layer + output) are ALL Q4_0 has their blocks registered
 *   as they are (lh_tensor_register dtype 2: every nibble kept, n = 0 included); any other file loads exactly as llama_LoadModel loads it. */
int llamago_QuantizeModelQ4(llama_model* m);
int llamago_ExpandModelQ4(llama_model* m);
int llamago_SaveModelQ4(const llama_model* m, const char* fileName);
llama_model* llamago_LoadModelKeepQ4(const char* fileName, uint32_t ctxSize);

/* ---- [product] harness helper of the kept decode graph (no GPU needed) -------------------------------------------------- */
/* The array llama_Eval hands to lh_graph_compute for N tokens (ids 1..N) at pastQuery, as numbers: per tensor 16 int64 = op, dtype, flags, ne[4],
 * nb[4], src0, src1, storage, view_off, a fold of an owner leaf's host values (0 without).  pastBuild < 0: from a fresh build at pastQuery;
 * pastBuild >= 0: from the graph llama_Eval KEEPS between one-token calls, learnt around pastBuild and moved to pastQuery (host/llamago.cpp,
 * eval_cache) - tests require both to be identical.  Returns the tensor count, -1 bad arguments, -2 the kept graph declined. */
int llamago_DescribeEvalArray(const llama_hparams* hp, uint32_t ctxSize, uint32_t N, int64_t pastBuild, uint32_t pastQuery, int64_t* out, uint32_t cap_tensors, uint32_t* n_leafs);
/* Flattened graphs as real lh_tensor records with storage, view_off and buf - what lh_graph_check takes.  Host values (token ids, op parameters,
 * caller-filled leafs) are copied to host_vals, where the records' host pointers then point.  Both return the tensor count; out = NULL asks for
 * the counts only; -1 on bad arguments or arrays that are too small.
 * llamago_GraphRecords: any graph built with the mirror's constructors (ctx = NULL serves all of them).
 * llamago_EvalGraphRecords: the graph llama_Eval builds for N tokens (ids 1..N) at pastCount, built fresh; every weight and cache of the shape model
 * gets a buffer id of its own (1, 2, ...) and an lh_buf_extent that says what a registration of it would hold. */
int llamago_GraphRecords(ml_graph* g, lh_tensor* out, uint32_t cap_tensors, uint32_t* n_leafs, float* host_vals, uint32_t cap_vals, uint32_t* n_vals);
int llamago_EvalGraphRecords(const llama_hparams* hp, uint32_t ctxSize, uint32_t N, uint32_t pastCount, lh_tensor* out, uint32_t cap_tensors, uint32_t* n_leafs,
                             lh_buf_extent* bufs, uint32_t cap_bufs, uint32_t* n_bufs, float* host_vals, uint32_t cap_vals, uint32_t* n_vals);
/* 0: every llama_Eval builds its graph anew (what LLAMAGO_NO_EVAL_CACHE=1 sets at load); 1 (default): one-token Evals move the kept graph. */
void llamago_KeepDecodeGraph(int on);

/* ---- [product] device-resident loops on a llama.Context --------------------------------------------------------------- */
/* n_steps greedy decode steps without host round trips (lh_llama_decode_greedy). */
int llamago_DecodeGreedyResident(llama_context* c, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t* out_tokens, float* logits_last);
/* HIP-event timing of every kernel class of one decode step (lh_llama_profile_decode); returns the class count. */
int llamago_ProfileDecode(llama_context* c, uint32_t token, uint32_t past, uint32_t repeats, lh_kernel_time* out, uint32_t cap);
/* One pipeline stage of Eval on the context's own KV cache (lh_llama_stage). */
int llamago_Stage(llama_context* c, const uint32_t* tokens, const void* tokens_dev, const void* x_in_dev, void* x_out_dev, uint32_t n, uint32_t past,
                  void* logits_dev, void* argmax_dev);
/* lh_score_rows on the model context's device: rows of host logits [n_rows][n_logits] scored against targets[row] (op-level parity). */
int llamago_ScoreRows(const float* logits, uint32_t n_rows, uint32_t n_logits, const uint32_t* targets, lh_row_score* out);
/* lh_argmax_rows on the model context's device: the greedy id of every row of host logits [n_rows][n_logits], by k_argmax_advance launched once per
 * row (which = 0) or by one k_batch_argmax launch over all rows (which = 1) - the two kernels every greedy route takes its ids from (op-level parity). */
int llamago_ArgmaxRows(const float* logits, uint32_t n_rows, uint32_t n_logits, int which, uint32_t* ids_out);
/* lh_llama_score on the context's own KV cache: llama.Eval of tokens[0..n) at pastCount with the lm_head for all n rows (llama.go:384), every row
 * reduced on the device (softmax arithmetic llama.go:581-609); out[i] belongs to the logits behind tokens[i].  targets_or_null == NULL: row i against
 * tokens[i+1], the last row against its own greedy id.  Leaves the cache as llama_Eval with the same arguments does. */
int llamago_Score(llama_context* c, llama_model* m, const uint32_t* tokens, uint32_t n, uint32_t pastCount, const uint32_t* targets_or_null, lh_row_score* out);
/* Perplexity of a token sequence.  Convention: the sequence is cut into consecutive windows of ctxSize tokens (the last one shorter; a window of
 * one token is dropped); each window starts at position 0 and is evaluated in Evals of at most `chunk` rows (chunk = 0: 512) with advancing
 * pastCount; row i of a window is scored against token i+1 of the window, the window's last row is not scored.  nll_sum = -sum logprob in f64,
 * n_scored = the number of terms; perplexity = exp(nll_sum / n_scored).  The context's cache holds the last window afterwards. */
int llamago_Perplexity(llama_context* c, llama_model* m, const uint32_t* tokens, uint32_t n_tokens, uint32_t chunk, double* nll_sum, uint64_t* n_scored);
/* Lookup-draft speculative decoding (lh_draft_lookup, lh_llama_verify, lh_llama_decode_lookup; the rule is stated in llamahip.h).
 * llamago_DraftLookup: the drafter alone on host arrays, on the model context's device.  llamago_Verify: one verify pass of tokens[0..n) (pending
 * token + a draft from anywhere) on the context's own KV cache.  llamago_DecodeLookup: llamago_DecodeGreedyResident through verify passes - the
 * same ids, the same last logits, the same state left behind. */
int llamago_DraftLookup(const uint32_t* window, uint32_t n_window, const lh_lookup_params* lp, uint32_t limit, uint32_t* draft_out, uint32_t* n_draft);
int llamago_Verify(llama_context* c, const uint32_t* tokens, uint32_t n, uint32_t past, uint32_t* ids_out, uint32_t* n_accepted, float* logits);
int llamago_DecodeLookup(llama_context* c, uint32_t first_token, uint32_t past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out_tokens,
                         float* logits_last, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);
/* Draft-model speculative decoding (lh_llama_decode_draft; the rule, the state left behind and the refusals are stated in llamahip.h): a second model
 * drafts, the target verifies, the ids are those of llamago_DecodeGreedyResident on the target.  llama_NewContext makes one lh_ctx per context and the loop
 * needs both plans on one stream, so a PAIR creates its two contexts (one KV cache each, ctxSize positions) over one ml.Context.
 * llamago_DraftPairTarget / llamago_DraftPairDraft hand them out as ordinary llama_context*: llama_Eval, llama_GreedyDecode, llamago_DecodeLookup and the rest
 * work on them (one at a time: they share a stream); they belong to the pair - never pass them to llama_ReleaseContext.  The caller evaluates the prompt on
 * BOTH before llamago_DecodeDraft (the precondition of lh_llama_decode_draft).  llamago_DraftPairReplaceDraft frees the draft context and makes a fresh
 * one (an empty cache) over another model; the target context stays.  llamago_FreeDraftPair frees both contexts; the models stay the caller's.
 * llamago_DecodeDraftContexts is the call underneath on any two contexts: those of a pair, or - to be refused - two that do not share a stream, or the same
 * one twice.  Both Decode calls return 0 or a NEGATIVE LH_E* code, never 1 (the other llamago_* entry points return 1): the code of lh_llama_decode_draft, LH_EINVAL for a
 * null pair or context, LH_EHIP when a context's stage could not be made (message: ml_LastError).  A caller tells a refusal (LH_EINVAL, LH_EUNSUPPORTED: both
 * contexts untouched) from a failure by it. */
typedef struct llama_draft_pair llama_draft_pair;
llama_draft_pair* llamago_NewDraftPair(llama_model* target_model, llama_model* draft_model, uint32_t ctxSize);
void llamago_FreeDraftPair(llama_draft_pair* p);
llama_context* llamago_DraftPairTarget(llama_draft_pair* p);
llama_context* llamago_DraftPairDraft(llama_draft_pair* p);
int llamago_DraftPairReplaceDraft(llama_draft_pair* p, llama_model* draft_model);
int llamago_DecodeDraft(llama_draft_pair* p, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t draft_len, uint32_t* out_tokens, float* logits_last,
                        lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);
int llamago_DecodeDraftContexts(llama_context* target, llama_context* draft, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t draft_len,
                                uint32_t* out_tokens, float* logits_last, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);
/* The same for sampled generation (lh_sample_rows, lh_llama_decode_sample_lookup; ring view, draw and commit per row are stated in llamahip.h).
 * llamago_SampleRows: the multi-row sampler alone on host arrays, on the model context's device - row r of logits [n_rows][n_logits] sampled as
 * call draw0 + r over the ring behind tokens[1..r].  llamago_SampleDecodeLookup: llama_SampleDecode through verify passes that sample every row -
 * the same ids, the same state left behind; ring_size = 0 means ctxSize, the reference's ring (server.go:127). */
int llamago_SampleRows(const float* logits, uint32_t n_rows, uint32_t n_logits, const uint32_t* ring, uint32_t ring_size, uint32_t ring_pos, const uint32_t* tokens,
                       uint32_t topK, float topP, float temp, float repeatPenalty, uint64_t seed, uint64_t draw0, uint32_t* ids_out);
int llamago_SampleDecodeLookup(llama_context* c, llama_model* m, const uint32_t* prompt, uint32_t n_prompt, uint32_t n_predict, uint32_t ring_size, uint32_t topK,
                               float topP, float temp, float repeatPenalty, uint64_t seed, const lh_lookup_params* lp, uint32_t* out_tokens, lh_spec_stats* stats,
                               uint16_t* trace, uint32_t trace_cap);

/* ModelParams.Embedding (llama.go:52, 88): from now on every llama_Eval also leaves row N-1 of `embeddings` (the final norm * weight rows,
 * llama.go:381, 414-419) in lctx.Embedding; llama_Embedding (llamago.h) returns it ([embd] floats; NULL when not enabled).  On the GPU the fused plan
 * never writes those rows out by itself: the Eval graph's node is flagged LH_T_OUTPUT. */
void llamago_EnableEmbedding(llama_context* c);
/* ModelParams.KeepCount (llama.go:47): the tokens a context swap keeps (server.go:166-167); 0 in the reference's own main.go.  The generation
 * loops (llama_GreedyDecode, llama_SampleDecode, llamago_DecodeGreedyResident) swap context at the window's end as server.Do does. */
void llamago_SetKeepCount(llama_context* c, uint32_t keep);

/* ---- [product] the pods of one GPU in ONE weight pass (lh_batch; server.go:88-101, 151) ------------------------------- */
typedef struct llama_batch llama_batch;
/* `pods` llama.Contexts (one KV cache each, llama.go:91-103) over one whole Model on one stream, bound into an lh_batch. */
llama_batch* llamago_NewBatch(llama_model* m, uint32_t ctxSize, uint32_t pods);
void llamago_FreeBatch(llama_batch* b);
int llamago_BatchBatched(llama_batch* b);            /* lh_batch_batched */
int llamago_BatchSetF16Stream(llama_batch* b, int on);   /* llamago_SetF16Stream on the lh_ctx the batch evaluates in */
int llamago_BatchF16Stream(llama_batch* b);
int llamago_BatchSetQ4Stream(llama_batch* b, int on);    /* llamago_SetQ4Stream on the lh_ctx the batch evaluates in */
int llamago_BatchQ4Stream(llama_batch* b);
/* Test instrumentation: llamago_CacheRead / llamago_CacheWrite on the KV cache of pod `pod` (also fails on a pod outside the batch). */
int llamago_BatchCacheRead(llama_batch* b, uint32_t pod, int which, uint64_t off_floats, float* dst, uint64_t n);
int llamago_BatchCacheWrite(llama_batch* b, uint32_t pod, int which, uint64_t off_floats, const float* src, uint64_t n);
int64_t llamago_BatchPoisonWeightImages(llama_batch* b);   /* llamago_PoisonWeightImages on the lh_ctx the batch evaluates in */
/* Every pod: its prompt as one Eval, then n_predict - 1 greedy steps of ALL pods per weight pass.  out[i * n_predict + s] = s-th id
 * of pod i (= llama_GreedyDecode of that prompt alone); logits (optional): [pods][vocab] of the last tick. */
int llamago_BatchGreedyDecode(llama_batch* b, const uint32_t* const* prompts, const uint32_t* n_prompt, uint32_t n_predict, uint32_t* out, float* logits);
/* The twins of the Go shim's BatchHIP.Prompt / BatchHIP.Tick (go/ml_hip_pods.go): every pod's prompt as one Eval / one decode step of every pod
 * in one pass over the weights; ids_out[pods] = the ids produced.  A tick that would leave a pod's context window is an error
 * (llama.Eval's pastCount + N <= CtxSize), never a write past its KV cache. */
void llamago_BatchSetKeepCount(llama_batch* b, uint32_t keep);   /* ModelParams.KeepCount of every pod (see llamago_SetKeepCount) */
int llamago_BatchPrompt(llama_batch* b, const uint32_t* const* prompts, const uint32_t* n_prompt, uint32_t* ids_out);
int llamago_BatchTick(llama_batch* b, uint32_t* ids_out);
int llamago_BatchSet(llama_batch* b, const uint32_t* tokens_or_null, const uint32_t* past);   /* lh_batch_set: token and position of every pod's next tick */
/* lh_batch_feed: llama.Eval for any subset of the pods, packed into shared weight passes - prompts of new jobs, next turns, chunks of long prompts
 * and decode rows ride one pass over the weights.  Pod i evaluates tokens[i][0..n_tokens[i]) at position past[i] of its own cache; n_tokens[i] == 0:
 * not fed.  A fed pod's next tick evaluates the greedy id of its last fed row (ids_out[i]); the other pods go on as if nothing had happened.
 * Optional outputs: ids_out [pods], logits_last [pods][vocab] (fed pods' entries only), logits_rows [sum n_tokens][vocab] (pods in index order). */
int llamago_BatchFeed(llama_batch* b, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past, uint32_t* ids_out, float* logits_last,
                      float* logits_rows);
/* lh_batch_set_sampler on the batch: the following ticks pick every pod's id with SampleTopPTopK (llama.go:455-707) instead of the argmax, every
 * pod seeded like a solo run; ringSize slots of lastNTokens per pod, empty.  May be called mid-stream (behind llamago_BatchPrompt and ticks). */
int llamago_BatchSetSampler(llama_batch* b, uint32_t topK, float topP, float temp, float repeatPenalty, uint64_t seed, uint32_t ringSize);
int llamago_BatchClearSampler(llama_batch* b);   /* lh_batch_set_sampler(NULL): the following ticks take the argmax again */
/* lh_batch_feed_sample: llamago_BatchFeed on a batch whose ticks sample - a job joins (flags[i] = LH_FEED_NEW: pod i's ring and draw counter restart, its
 * prompt in ONE feed), a pod takes a next turn (0) or its own pending id (LH_FEED_PENDING) while the other pods go on sampling.  Every fed pod's last row
 * is sampled over its ring behind the fed tokens (the rule is stated in llamahip.h); ids_out[i] = that id, which the pod's next tick evaluates.
 * flags NULL = all 0.  llamago_BatchFeed on such a batch stays refused. */
int llamago_BatchFeedSample(llama_batch* b, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past, const uint32_t* flags, uint32_t* ids_out,
                            float* logits_last, float* logits_rows);
/* lh_batch_decode_lookup: n_steps greedy ids per pod from (first_tokens[i], past[i]) through lookup-drafted verify passes of pods x R rows (the rule,
 * the window condition past + n_steps + R - 1 <= ctxSize and the state left behind are stated in llamahip.h).  out [pods][n_steps]; optional: logits_last
 * [pods][vocab] (the logits behind each pod's last id), stats [pods], trace [pods][trace_cap].  llamago_SpecAcceptPods: lh_spec_accept_pods, the accept
 * step of such a pass alone on host arrays, on the model context's device. */
int llamago_BatchDecodeLookup(llama_batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out,
                              float* logits_last, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);
int llamago_SpecAcceptPods(const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos, const uint32_t* produced,
                           uint32_t n_steps, uint32_t ctx_size, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out, uint32_t* pending_out, uint32_t* ids_out);
/* The same on a batch behind llamago_BatchSetSampler (lh_batch_decode_sample_lookup, lh_sample_pod_rows, lh_spec_accept_sample_pods, lh_batch_sampler_read;
 * the rule per pod and the contract are stated in llamahip.h): the generation loop of server.go:201-217 for every pod through verify passes whose pods x R
 * rows are sampled in one launch (SampleTopPTopK, llama.go:455-707) - the ids, rings and draw counters of llamago_BatchDecode on the same batch.
 * llamago_SamplePodRows / llamago_SpecAcceptSamplePods: that sampler launch / the accept step with the ring commit (appendToken, server.go:205) alone on host
 * arrays, on the model context's device.  llamago_BatchSamplerRead: pod `pod`'s ring (llamago_BatchSamplerRingSize(b) entries - the ringSize of the last
 * llamago_BatchSetSampler, 0 without a sampler; server.go:127-138), ids appended so far and next sampling call; each output optional. */
int llamago_BatchDecodeSampleLookup(llama_batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out,
                                    float* logits_last, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);
int llamago_SamplePodRows(const float* logits, uint32_t n_pods, uint32_t n_rows, uint32_t n_logits, const uint32_t* rings, uint32_t ring_size, const uint32_t* ring_pos,
                          const uint64_t* draws, const uint32_t* tokens, const uint32_t* n_draft, uint32_t topK, float topP, float temp, float repeatPenalty,
                          uint64_t seed, uint32_t* ids_out);
int llamago_SpecAcceptSamplePods(const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos,
                                 const uint32_t* produced, uint32_t n_steps, uint32_t ctx_size, const uint32_t* rings, uint32_t ring_size, const uint32_t* ring_pos,
                                 const uint64_t* draws, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out, uint32_t* pending_out, uint32_t* ids_out,
                                 uint32_t* rings_out, uint32_t* ring_pos_out, uint64_t* draws_out);
uint32_t llamago_BatchSamplerRingSize(llama_batch* b);
int llamago_BatchSamplerRead(llama_batch* b, uint32_t pod, uint32_t* ring_out, uint32_t* ring_pos_out, uint64_t* draw_out);
/* lh_batch_decode: n_steps ticks of every pod from (first_tokens[i], past[i]) in one call; out [pods][n_steps], logits_last (optional) [pods][vocab]:
 * the logits of the last tick (llamago_BatchTick returns ids only). */
int llamago_BatchDecode(llama_batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, uint32_t* out, float* logits_last);
/* lh_batch_fork: cache rows [0, n_pos) of every layer, K and V, and the token history of pod src copied into the pods dst[0..n_dst), which then form a
 * sharing group of length n_pos with src: the ticks read the group's prefix once per block of member rows, every logit byte-equal to a batch that never
 * forked (the rule, the leave predicate, the refusals and what is out of scope are stated in llamahip.h).  Nothing else moves: feed each destination at
 * past = n_pos or place it with llamago_BatchSet.  llamago_BatchCacheWrite into rows below the shared length makes the pod leave its group.
 * llamago_BatchShareInfo: lh_batch_share_info - per pod the lowest pod of its group and the shared length (its own index and 0 without a group).
 * llamago_ShareSchedule: lh_share_schedule, the block table a tick derives from that state, alone on host arrays (no GPU). */
int llamago_BatchFork(llama_batch* b, uint32_t src, const uint32_t* dst, uint32_t n_dst, uint32_t n_pos);
int llamago_BatchShareInfo(llama_batch* b, uint32_t* group, uint32_t* len);
int llamago_ShareSchedule(const uint32_t* group, const uint32_t* len, uint32_t rows, uint32_t qb, uint32_t min_rows, lh_share_block* blocks, uint32_t cap,
                          uint32_t* row_block);
/* lh_sample_pods: the multi-pod sampler of a sampled tick alone on host arrays, on the model context's device - row i of logits [n][n_logits] over ring i
 * of rings [n][ring_size] (ring_pos[i] ids appended so far) as sampling call draws[i]; rings_out / ring_pos_out (optional) = the rings behind the ids. */
int llamago_SamplePods(const float* logits, uint32_t n, uint32_t n_logits, const uint32_t* rings, uint32_t ring_size, const uint32_t* ring_pos, const uint64_t* draws,
                       uint32_t topK, float topP, float temp, float repeatPenalty, uint64_t seed, uint32_t* ids_out, uint32_t* rings_out, uint32_t* ring_pos_out);

/* ---- [product] pods as pipeline streams over a layer-sharded model ---------------------------- */
typedef struct llama_pipeline llama_pipeline;
int llamago_CommUniqueId(uint8_t* id /* [LH_COMM_ID_BYTES] */);   /* lh_comm_unique_id on this process's device: rank 0 calls, any channel distributes */
/* This rank's stages of `pods` independent streams over the model's [layer0, layer1) (llama_NewSyntheticModel / loader with a layer
 * range), one KV cache per stream, one HIP stream per rank.  id = the 128 bytes from rank 0 (RCCL), or NULL with hooks (host-staged
 * transport), or both NULL for an unsharded model (world 1).  maxRows (Grouped): streams one tick evaluates together in one pass over
 * the rank's weights; 0 = as many as fit, 1 = every stream on its own. */
llama_pipeline* llamago_NewPipeline(llama_model* m, uint32_t ctxSize, uint32_t pods, int rank, int world, const uint8_t* id, const lh_comm_hooks* hooks);
llama_pipeline* llamago_NewPipelineGrouped(llama_model* m, uint32_t ctxSize, uint32_t pods, int rank, int world, const uint8_t* id, const lh_comm_hooks* hooks,
                                           uint32_t maxRows);
void llamago_FreePipeline(llama_pipeline* p);
uint32_t llamago_PipelineGroups(llama_pipeline* p);
int llamago_PipelineRun(llama_pipeline* p, const uint32_t* const* prompts, const uint32_t* n_prompt, uint32_t steps);             /* lh_pipeline_run */
int llamago_PipelineRunSample(llama_pipeline* p, const uint32_t* const* prompts, const uint32_t* n_prompt, uint32_t steps, uint32_t topK, float topP, float temp,
                              float repeatPenalty, uint64_t seed, uint32_t ringSize);                                            /* lh_pipeline_run_sample */
int llamago_PipelineSetKeepCount(llama_pipeline* p, uint32_t keep);                                               /* lh_pipeline_set_keep (same value on every rank) */
int llamago_PipelineProfile(llama_pipeline* p, int on);                                                          /* lh_pipeline_profile */
int llamago_PipelineStats(llama_pipeline* p, uint32_t* ticks, float* stage_ms, float* exchange_ms);             /* lh_pipeline_stats_read */
int llamago_PipelineHopProbe(llama_pipeline* p, uint32_t bytes, uint32_t iters, float* us_per_hop);             /* lh_pipeline_hop_probe */
int llamago_PipelineTokens(llama_pipeline* p, uint32_t pod, uint32_t* out, uint32_t cap);                                        /* lh_pipeline_tokens */
int llamago_PipelineProfileDecode(llama_pipeline* p, uint32_t token, uint32_t past, uint32_t repeats, lh_kernel_time* out, uint32_t cap);
int llamago_PipelineSync(llama_pipeline* p);

#ifdef __cplusplus
}
#endif
#endif
