/* include/llamahip.h — the drop-in C-ABI boundary of the MI355X backend (libllamahip.so).
 *
 * The reference (gotzmann/llama.go) has no plugin/FFI interface; the call that keeps its
 * ml.Tensor / ml.Graph operator surface intact and crosses Go -> C once per Eval is
 * ml.GraphCompute (pkg/ml/ml.go:1411-1528, called from pkg/llama/llama.go:389).  Every entry point
 * below is what a cgo shim inside package ml binds (INTEGRATION.md shows that shim); each cites the
 * reference interface it replaces.  Plain C: opaque handles, pointers and sizes, no torch/HIP types
 * (a HIP stream is passed as void*).
 *
 * Conventions
 *  - every function returns 0 on success or a negative LH_E* code and never aborts the process
 *    (the reference os.Exit(1)s on "[HALT]" conditions, e.g. ml.go:1538, 2116-2124; the shim maps a
 *    non-zero code back to that behaviour).  lh_last_error() returns the message.
 *  - thread-agnostic: a Go goroutine may migrate between OS threads between calls, so every entry
 *    point re-selects its device and uses the context's explicit stream.  One lh_ctx must not be
 *    used from two threads at once (the reference has one ml.Context per pod, server.go:151);
 *    registered weight buffers are shared read-only by all contexts of a device (server.go:45).
 *  - blocking: lh_graph_compute returns after the results are visible to lh_node_read, matching the
 *    wg.Wait() join of the reference (ml.go:1652).
 *  - no host pointer is retained past the call that received it (cgo pointer rule): weights are
 *    copied to HBM at registration.
 *  - ordering: an entry point that reads or writes HOST memory (uploads, reads, prompts, produced ids,
 *    logits) returns after the context's stream has drained; one that only takes DEVICE pointers
 *    (lh_llama_stage, lh_batch_stage, lh_comm_exchange over RCCL) enqueues on the context's stream and
 *    returns.  The private stream is non-blocking, i.e. NOT ordered with the null stream: the library
 *    itself waits for its stream before any synchronous (null-stream) copy, and a caller that touches
 *    the same buffers from another stream orders that stream against lh_ctx_stream() itself.
 */
#ifndef LLAMAHIP_H
#define LLAMAHIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LH_ABI_VERSION 1

enum { LH_OK = 0, LH_EINVAL = -1, LH_ENOMEM = -2, LH_EHIP = -3, LH_EUNSUPPORTED = -4, LH_ENODEVICE = -5, LH_ESHAPE = -6 };

typedef struct lh_ctx lh_ctx;   /* device side of one ml.Context (ml.go:50-57): stream, scratch arena, cached plans */
typedef uint64_t lh_buf;        /* handle of a persistent device buffer (weights, KV cache); 0 = none */

/* ---- contexts:  ml.NewContext ml.go:59-74 / (*Context).ReleaseContext ml.go:77-80 ------------- */
int lh_abi_version(void);
int lh_device_count(void);                      /* 0 when no GPU is visible (never an error) */
/* stream: an existing hipStream_t to enqueue on (e.g. the framework's current stream), or NULL for a
 * private non-blocking stream. */
int lh_ctx_create(int device, void* stream, lh_ctx** out);
void lh_ctx_destroy(lh_ctx* ctx);
const char* lh_last_error(lh_ctx* ctx);         /* ctx may be NULL: last error of the calling thread */
int lh_ctx_sync(lh_ctx* ctx);                   /* wait for everything enqueued on the context's stream */
/* Measurement aid: GB/s of a read-only stream over `bytes` of HBM (16-byte non-temporal loads, eight per lane in flight, one workgroup
 * per CU: the decode weight stream's access pattern with no arithmetic behind it) = what this box's memory delivers to a kernel that
 * does nothing else; the yardstick bench.py reports next to the nominal 8 TB/s (SURVEY 8d "vs measured achievable"). */
int lh_hbm_read_probe(lh_ctx* ctx, uint64_t bytes, uint32_t repeats, float* gbps);
void* lh_ctx_stream(lh_ctx* ctx);

/* ---- persistent tensors: weights resident after LoadModel (llama.go:975), KV cache of NewContext
 *      (llama.go:91-98).  `key` is a caller-chosen stable id (the Go shim uses the address of the
 *      tensor's backing array); registering an existing key returns the existing buffer.  key 0 =
 *      anonymous.  dtype is ml.DType (ml.go:85-94): 0 = f32; 1 = f16 (ml.TYPE_F16, weight matrices only:
 *      host = ne0 * ne1 uint16 halves, row-major [ne1][ne0], kept as halves in device memory); 2 = block-int4
 *      (ml.TYPE_Q4_0, weight matrices only: host = ne0 * ne1 / 32 blocks of 20 bytes {float d; uint8 qs[16]}, w = d * (n - 8),
 *      element 2j in the low nibble of qs[j]; ne0 = cols, a multiple of 32, ne1 = rows; every nibble is kept); 7 = block-int8
 *      (ours).  host may be NULL (buffer zero-filled, as Go's make([]float32) is).  lh_buf_nfloats of a
 *      dtype-1, dtype-2 or dtype-7 buffer is its logical element count; lh_buf_upload, lh_buf_read and
 *      lh_buf_fill_synth refuse a dtype-1 buffer (LH_EINVAL); lh_buf_upload and lh_buf_fill_synth refuse a
 *      dtype-2 buffer (LH_EINVAL), lh_buf_read returns its fl32(d * q) as for dtype 7. ------------- */
int lh_tensor_register(lh_ctx* ctx, uint64_t key, int dtype, const uint32_t ne[4], int persistent,
                       const void* host_or_null, lh_buf* out);
int lh_buf_upload(lh_ctx* ctx, lh_buf buf, uint64_t off_floats, const float* host, uint64_t n);
int lh_buf_read(lh_ctx* ctx, lh_buf buf, uint64_t off_floats, float* dst, uint64_t n);
/* Fill with the synthetic-model generator: w[i] = offset + scale * u(seed, tensor_id, i), in HBM. */
int lh_buf_fill_synth(lh_ctx* ctx, lh_buf buf, uint64_t off_floats, uint64_t n, uint64_t seed, uint32_t tensor_id,
                      float scale, float offset);
/* Block-int8 (dtype 7; our format — the reference has none, ml.go:85-94, llama.go:956-959): quantise a registered fp32
 * matrix [rows][cols] on the device into a new buffer (d = max|w|/127 per 32 columns, q = rint(w/d)).  A dtype-7 buffer
 * can also be registered directly from 36-byte interchange blocks {float d; int8 q[32]} with lh_tensor_register. */
int lh_buf_quantize_q8(lh_ctx* ctx, lh_buf src_f32, uint32_t rows, uint32_t cols, lh_buf* out);   /* a dtype-1 or dtype-2 source: LH_EUNSUPPORTED (quantise before narrowing; lh_buf_expand_q4) */
/* Block-int4 (dtype 2).  lh_buf_quantize_q4: a registered fp32 matrix [rows][cols], cols % 32 == 0, quantised on the device (k_quantize_q4) into a new
 * dtype-2 buffer: d = fl32(max|w| / 7) per 32 columns, q = clamp(rint(fl32(w / d)), -7, 7) (d = 0 -> q = 0; a block with a NaN or an infinity: d = NaN,
 * q = 0), stored as n = q + 8.  An f16, block-int8 or block-int4 source: LH_EUNSUPPORTED, the message names it.
 * lh_buf_expand_q4: a dtype-2 buffer as a new dtype-7 buffer with the same q and the same d (k_expand_q4; nothing is requantised): the two hold
 * identical values, and the decode kernels over either give identical bits.  A source of another dtype: LH_EINVAL.  Both synchronise. */
int lh_buf_quantize_q4(lh_ctx* ctx, lh_buf src_f32, uint32_t rows, uint32_t cols, lh_buf* out);
int lh_buf_expand_q4(lh_ctx* ctx, lh_buf src_q4, lh_buf* out_q8);
/* The 20-byte interchange blocks [block0, block0 + nblocks) of a dtype-2 buffer, exactly as lh_tensor_register takes them (for saving a model). */
int lh_buf_read_q4(lh_ctx* ctx, lh_buf buf, uint64_t block0, void* dst_blocks, uint64_t nblocks);
/* f16 (dtype 1).  lh_buf_narrow_f16: a registered fp32 matrix [rows][cols] converted on the device (k_narrow_f16) into a new dtype-1 buffer: round to
 * nearest even, overflow to +-inf, -0 kept; *n_changed (optional) = the elements whose value changed (0 for anything that came from an f16 file).
 * lh_buf_widen_f16: a dtype-1 buffer widened into a new fp32 buffer (k_widen_f16, the pass the prompt routes of an f16 model run in front of their
 * fp32 kernels); exact for every half, a NaN stays a NaN.  Both synchronise.  A source of the wrong dtype: LH_EINVAL. */
int lh_buf_narrow_f16(lh_ctx* ctx, lh_buf src_f32, uint32_t rows, uint32_t cols, lh_buf* out, uint64_t* n_changed);
int lh_buf_widen_f16(lh_ctx* ctx, lh_buf src_f16, lh_buf* out_f32);
/* f16 models on the weight-stream MFMA kernels of 2..128 rows (csrc/kernels_stream_f16.h).  lh_ctx_set_f16_stream(ctx, on): with on != 0 every Eval of an
 * f16 plan of this context that takes the prefill route hands the stream launches the model's own halves (k_stream_mm2_h / k_stream_dma_h) and widens a
 * matrix only directly in front of a launch that reads fp32 - it replaces the k_widen_f16 pass per matrix and layer in front of the fp32 stream kernels
 * (weight_dtype below), byte for byte the same results.  Off by default; the initial value is LLAMAHIP_F16_STREAM=1 of the environment, read once in
 * lh_ctx_create.  Read at every Eval; accepted and without effect for fp32, block-int8 and block-int4 plans.  A change makes every captured graph of an f16
 * plan on the context that may hold a stream launch run eagerly once and be captured anew.  lh_ctx_f16_stream: the current value (0 | 1; ctx NULL: 0). */
int lh_ctx_set_f16_stream(lh_ctx* ctx, int on);
int lh_ctx_f16_stream(lh_ctx* ctx);
/* Where k_stream_dma_h keeps a half (csrc/stream_f16_layout.h; pure host functions, for checks): byte offset, in the weight part of a ring image of
 * kc-column chunks (64 | 128), of 16-byte granule g (columns 8 g .. 8 g + 7 of the chunk) of image row r (< 128) / of the 8 bytes MFMA lane (r16, slot) reads of
 * tile slot t (< 8) for k-block kb (< kc / 16) of the chunk.  An argument out of range: -1. */
int64_t lh_stream_f16_image_off(uint32_t kc, uint32_t r, uint32_t g);
int64_t lh_stream_f16_read_off(uint32_t kc, uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot);
/* f16 models on the bf16 tile GEMM of prompts beyond 128 rows (csrc/kernels_gemm_f16.h).  lh_ctx_set_f16_tiles(ctx, on): with on != 0 every k_gemm_b9 launch
 * of an f16 plan's prefill route reads the model's own halves (k_gemm_b9_h: six exact bf16 products instead of eight, no k_widen_f16 pass in front), where the
 * widened twin launches k_gemm_b9 and with its split count; every other launch of the route widens what it reads directly in front of itself.  Byte for byte
 * the same results.  Off by default; the initial value is LLAMAHIP_F16_TILES=1 of the environment, read once in lh_ctx_create.  Read at every Eval; accepted
 * and without effect for fp32, block-int8 and block-int4 plans; independent of lh_ctx_set_f16_stream.  No captured graph holds such a launch (more than 128
 * rows), so a change re-captures nothing.  lh_ctx_f16_tiles: the current value (0 | 1; ctx NULL: 0). */
int lh_ctx_set_f16_tiles(lh_ctx* ctx, int on);
int lh_ctx_f16_tiles(lh_ctx* ctx);
/* The pure pieces of k_gemm_b9_h (csrc/gemm_f16_layout.h; host functions, for checks).  lh_gemm_f16_split: *w = the fp32 bits of half h, *r1 = the bits of
 * w - (w & 0xffff0000): the kernel's hi / mid parts are their top 16 bits.  lh_gemm_f16_piece: DMA piece p (< 40) of a ring stage, lane (< 64): out = {byte
 * offset in the stage, tile row fetched (plane-local for p < 24), source granule of the row's 64 slab bytes}.  lh_gemm_f16_w_read_off: byte offset in the stage
 * of the 8 halves lane (li < 32, lh < 2) of wave wm (< 8) reads for k-step kk (< 2).  An argument out of range: -1. */
void lh_gemm_f16_split(uint16_t h, uint32_t* w, uint32_t* r1);
int lh_gemm_f16_piece(uint32_t p, uint32_t lane, uint32_t out[3]);
int64_t lh_gemm_f16_w_read_off(uint32_t wm, uint32_t li, uint32_t lh, uint32_t kk);
/* Block-int4 models on the bf16 stream kernel of 5..64 rows of a tick / 5..88 of a prompt (csrc/kernels_stream_q4b.h).  lh_ctx_set_q4_stream(ctx, on): with
 * on != 0 every Eval of a block-int4 plan of this context that takes the route over activation planes hands the k_stream_q8b launch sites the model's own
 * nibble planes and scale planes (k_stream_q4b) and enqueues no k_expand_q4 pass for a matrix that only such launches read; a launch that still reads int8
 * (prompts from 89 rows, a fallback) gets its matrix expanded directly in front of itself.  Byte for byte the same results: the schedule, every kernel
 * shape and every sum are the int8 twin's.  Off by default; the initial value is LLAMAHIP_Q4_STREAM=1 of the environment, read once in lh_ctx_create.  Read
 * at every Eval; accepted and without effect for fp32, f16 and block-int8 plans; independent of the f16 switches.  A change makes every captured graph of a
 * block-int4 plan on the context that may hold a stream launch run eagerly once and be captured anew.  lh_ctx_q4_stream: the current value (0 | 1; ctx NULL: 0). */
int lh_ctx_set_q4_stream(lh_ctx* ctx, int on);
int lh_ctx_q4_stream(lh_ctx* ctx);
/* Where k_stream_q4b keeps a nibble (csrc/stream_q4_layout.h; pure host functions, for checks): byte offset, in the weight part of a ring image of kc-column
 * chunks (128 | 256 | 512), of 16-byte granule g (quant block g: columns 32 g .. 32 g + 31 of the chunk) of image row r (< 128) / of the 4 bytes MFMA lane
 * (r16, slot) reads of tile slot t (< 8) for quant block kb (< kc / 32) of the chunk.  An argument out of range: -1.
 * lh_stream_q4_operand: the kernel's nibble -> bf16 conversion on the host - the eight nibbles of `nibbles` (nibble k = bits 4 k .. 4 k + 3) as the four
 * dwords of the MFMA operand (out[j] = the bf16 of n_2j - 8 in the low half, of n_2j+1 - 8 in the high half). */
int64_t lh_stream_q4_image_off(uint32_t kc, uint32_t r, uint32_t g);
int64_t lh_stream_q4_read_off(uint32_t kc, uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot);
void lh_stream_q4_operand(uint32_t nibbles, uint32_t out[4]);
/* Test instrumentation.  The context owns one fp32 (f16 plans) or int8 (block-int4 plans) image of ONE layer's matrices and one of the output matrix per plan
 * size; every route that reads an image fills the slots it reads in front of its own launches.  lh_ctx_poison_weight_images fills every such image with 0xFF
 * bytes (NaN as fp32, quant -1 as int8), enqueued on the context's stream, and stores the bytes filled (0: the context has no f16 or block-int4 plan).  A
 * launch that reads a slot its own call did not fill then computes from poison instead of from what the call before left there. */
int lh_ctx_poison_weight_images(lh_ctx* ctx, uint64_t* bytes);
/* Dequantised fp32 values of a dtype-7 buffer (w = fl32(d*q)), for checks. */
int lh_buf_read_q8(lh_ctx* ctx, lh_buf buf, uint64_t off, float* dst, uint64_t n);
int lh_buf_free(lh_ctx* ctx, lh_buf buf);
void* lh_buf_devptr(lh_ctx* ctx, lh_buf buf);   /* raw device address (interop with a framework's collectives) */
uint64_t lh_buf_nfloats(lh_ctx* ctx, lh_buf buf);

/* ---- the graph:  ml.GraphCompute ml.go:1411-1528 ---------------------------------------------------
 * One flat array describes Graph.Leafs (first n_leafs entries) then Graph.Nodes in execution order
 * (ml.go:42-44).  lh_tensor mirrors ml.Tensor (ml.go:180-203); op and dtype use the reference's
 * numeric values (ml.go:133-174, 85-94).  Go slices alias invisibly to C, so view identity is carried
 * explicitly: `storage` is the index of the tensor that owns the bytes (itself if it owns them) and
 * `view_off` the offset in floats from that owner's first element. */
typedef struct lh_tensor {
    uint8_t op;          /* ml.optype */
    uint8_t dtype;       /* ml.DType */
    uint16_t flags;      /* LH_T_* */
    uint32_t ne[4];      /* Tensor.NE */
    uint64_t nb[4];      /* Tensor.NB, bytes, widened to 64-bit (the reference's uint32 strides cap at 4 GiB) */
    int32_t src0, src1;  /* indices into this array, -1 = nil */
    int32_t storage;     /* owner index (== own index when this tensor owns its bytes) */
    uint32_t reserved;
    uint64_t view_off;   /* floats from the owner's base */
    lh_buf buf;          /* owner only: registered persistent buffer, or 0 for per-graph scratch */
    const float* host;   /* owner leaf with buf == 0: host data uploaded for this call (token ids, op params); else NULL */
} lh_tensor;

enum { LH_T_OUTPUT = 1 /* the host wants to read this node back with lh_node_read (in the reference every Tensor.Data is readable after
                           GraphCompute).  Node-by-node execution materialises everything anyway.  A fused plan materialises the final node and,
                           when flagged, llama.Eval's `embeddings` (the final norm rows, llama.go:381, 414-419); a graph with any other flagged
                           intermediate is executed node by node instead */ };
enum {
    LH_GRAPH_NO_FUSION = 1,        /* run every node 1:1 with the generic kernels (debug / op-level parity tests) */
    LH_GRAPH_LAST_ROW_LOGITS = 2   /* caller reads only row N-1 of the final MulMat (what llama.Eval does: it builds the
                                      lm_head for all N rows, llama.go:384, and copies out the last, llama.go:394-401): a
                                      fused plan then evaluates the lm_head for that row only and leaves rows 0..N-2 of the
                                      final node unwritten.  Ignored by the node-by-node path. */
};

int lh_graph_compute(lh_ctx* ctx, const lh_tensor* tensors, uint32_t n_leafs, uint32_t n_nodes, uint32_t flags);
/* What lh_graph_compute refuses before it enqueues anything, as a pure host function (csrc/graph_check.h; needs no context and no device): LH_OK,
 * or the negative code lh_graph_compute returns for this array, with the message in msg (cap bytes, may be NULL).  Two levels: the structural
 * checks every call makes (counts, storage owners, source indices and order, arity, strides that are whole floats, no extent of 0 - an empty
 * tensor is refused, not skipped), then what a node-by-node walk checks in front of its first launch: every op's shape rules and parameter leafs
 * and the furthest float its kernel touches in every operand, which must lie inside the owner.  bufs names what the registered buffers the array
 * refers to hold (lh_buf_nfloats; dtype as at registration); a host leaf holds its nelem floats, any other owner its own strided span. */
typedef struct lh_buf_extent { lh_buf id; uint64_t nfloats; int dtype; } lh_buf_extent;
int lh_graph_check(const lh_tensor* tensors, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, char* msg, uint64_t cap);
/* The gate of lh_graph_compute as a pure host function (csrc/graph_match.h; needs no context and no device): 1 when the array is recognised as
 * the graph llama.Eval builds and would run as the fused plan, 0 when it would run node by node, or the negative code of the structural checks.
 * lh_graph_compute runs the same matcher over its buffer table; here bufs says what the registered buffers hold, as for lh_graph_check.  An
 * extent carries no rows / cols, so a block-int8 (dtype 7) weight must hold exactly ne0 * ne1 logical elements here, where the device entry
 * compares the rows and cols of the quantised buffer.  On 1, *out (may be NULL) receives everything the fused result depends on besides the
 * data: the geometry, N and past, the cache owners, the token leaf, llama.Eval's `embeddings` node, and the leaf index of every weight -
 * weights[9 * layer + k] for k = attention_norm, wq, wk, wv, wo, ffn_norm, w1, w2, w3, then tok_embeddings, norm, output.  n_weights is set to
 * 9 * L + 3; at most cap_weights entries are written (weights may be NULL). */
typedef struct lh_match_info {
    uint32_t N, past, V, d, H, hd, L, F, ctx;
    int32_t wtype;
    int32_t kc_owner, vc_owner, tokens_leaf, emb_node;
    int32_t* weights;
    uint32_t cap_weights, n_weights;
} lh_match_info;
int lh_graph_match(const lh_tensor* tensors, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, lh_match_info* out);
/* Read elements of a tensor of the LAST computed graph (flat, in storage order from the tensor's first
 * element).  Replaces the host's direct reads of Tensor.Data after GraphCompute (llama.go:394-401). */
int lh_node_read(lh_ctx* ctx, uint32_t index, uint64_t off_floats, float* dst, uint64_t n);
/* 1 if the last lh_graph_compute ran as a fused LLaMA plan, 0 if node-by-node. */
int lh_last_graph_fused(lh_ctx* ctx);
/* Timing of a context's lh_graph_compute calls, the measurement SURVEY 8d config 2 names ("hipEvent around each lh_graph_compute"):
 * device_us = sum over the calls of the time between an event recorded on the stream when the call starts and one recorded behind its last
 * launch / copy; wall_us = sum of the host time spent inside the calls (validate, match, enqueue, the wait, the pinned copy of the row).
 * Off by default (two event records per call); lh_ctx_time_computes(ctx, on) zeroes the sums. */
typedef struct lh_compute_stats {
    uint64_t calls;
    double wall_us;
    double device_us;
} lh_compute_stats;
int lh_ctx_time_computes(lh_ctx* ctx, int on);
int lh_ctx_compute_stats(lh_ctx* ctx, lh_compute_stats* out);

/* Route log (test instrumentation, process-wide): while it is on, every kernel launch of the library notes the launched kernel's family - the
 * __global__'s name without template arguments.  tests/test_gpu_zz_routes.py switches it on for the whole GPU suite and asserts at the end that
 * every __global__ of the product sources was reached.  lh_route_log(1) clears the set and starts, lh_route_log(0) stops; lh_route_names writes the
 * names, newline-separated and NUL-terminated, into buf (up to cap bytes) and returns the number of bytes the full list needs. */
int lh_route_log(int on);
int64_t lh_route_names(char* buf, uint64_t cap);

/* Route trace (test instrumentation, per calling thread): while it is on, every matmul launch the thread enqueues appends the kernel's
 * INSTANTIATION - template arguments and, where the launch has one, the split-K factor: "k_gemm_glds<2,2,2,1>/s3", "k_gemm_b9/s1",
 * "k_gemv_cols<2,2,8>" - and the passes that belong to it ("k_split3_rows", "k_splitk_reduce"), in launch order, repeats included.
 * Two different instantiations never give the same string.  lh_route_trace(1) clears the list and starts, lh_route_trace(0) stops
 * (the list stays readable); lh_route_trace_read writes the list like lh_route_names.  Independent of the route log above.
 * The fused plan's attention launch sites record theirs too (tests/test_gpu_attention_bound.py): "k_attention/hd128/n1" ("k_attention/rows/..." when
 * every query row has its own cache and position), "k_attention_split/c9/n1" + "k_attention_combine/c9/n1" (c = key chunks), "k_attn_flash/uncut/p1" or
 * "k_attn_flash/cut/p3" + "k_attn_flash_combine/p3" (p = the most parts a block is cut into), and "attention_gemm/hd64/n70" in front of its four
 * launches (the QK GEMM's entry, "k_softmax_causal", "k_transpose_v", the PV GEMM's entry).  A launch replayed from a captured graph records nothing. */
int lh_route_trace(int on);
int64_t lh_route_trace_read(char* buf, uint64_t cap);

/* ---- convenience layer over the same fused plan executor (harnesses, bench, pipeline stages) ------
 * Describes the weights of llama.Model (llama.go:181-193) + one KV cache (llama.go:173-178) for the
 * layer range [layer0, layer1) held by this process. */
typedef struct lh_llama_layer { lh_buf attention_norm, wq, wk, wv, wo, ffn_norm, w1, w2, w3; } lh_llama_layer;
typedef struct lh_llama_desc {
    uint32_t vocab, embd, heads, layers, ff, ctx; /* whole-model hyper-parameters (llama.go:149-158, 761) */
    uint32_t layer0, layer1;                      /* this stage's layers; [0, layers) = whole model */
    lh_buf tok_embeddings, norm, output;          /* needed on the first / last stage only (0 elsewhere) */
    const lh_llama_layer* layer;                  /* `layers` entries, only [layer0, layer1) are read */
    lh_buf k_cache, v_cache;                      /* embd * (layer1-layer0) * ctx floats each; layer il at slot (il-layer0) */
    int weight_dtype;                             /* 0 = f32, 1 = f16, 2 = block-int4, 7 = block-int8 matrices; every matrix buffer must be of that dtype (f16: else LH_EINVAL).
                                                   * f16: one row and 2..8 rows stream the halves (k_gemv_sa_h / k_gemv_rows_h); every other row count runs the
                                                   * fp32 schedule over an fp32 image widened layer by layer - in all cases the bytes an fp32 model holding the
                                                   * same values produces */
} lh_llama_desc;
typedef struct lh_llama lh_llama;

int lh_llama_create(lh_ctx* ctx, const lh_llama_desc* desc, lh_llama** out);
void lh_llama_destroy(lh_llama* m);
/* llama.Eval (llama.go:211-426) on a whole model: logits of the last token to host (vocab floats). */
int lh_llama_eval(lh_llama* m, const uint32_t* tokens, uint32_t n, uint32_t past, float* logits_host);
/* ModelParams.KeepCount (llama.go:47) of this context: the first tokens a context swap keeps.  The generation loops below do what
 * server.Do does when the window is full (pkg/server/server.go:160-172: leftCount = pastCount - KeepCount; pastCount = KeepCount; the
 * last leftCount / 2 entries of lastNTokens - which already holds the pending token - are re-fed in front of it and evaluated as one
 * Eval): they go on generating instead of failing.  The swap needs the tokens of the window, which the context knows from the Evals
 * that went through it with host token ids and from its own resident loops; otherwise the loop fails with LH_EINVAL at the window's
 * end.  A single Eval past the window (lh_llama_eval, lh_llama_stage, lh_graph_compute) stays an error, as llama.Eval would panic. */
int lh_llama_set_keep(lh_llama* m, uint32_t keep);
/* The greedy rule of every route that picks ids on the device (lh_llama_decode_greedy, lh_llama_stage's argmax, lh_llama_verify,
 * lh_llama_decode_lookup, lh_batch_decode_lookup, lh_batch_tick / _prompt / _feed): lowest index on ties; NaN as the checker's argmax_f32, i.e. the reference's
 * `best = 0; if x[i] > x[best] { best = i }` loop - a NaN at index 0 wins the row, a NaN anywhere else is never taken.  +0 and -0 tie.
 * lh_argmax_rows is the op-level twin of lh_sample_top_p_top_k / lh_score_rows for the two kernels behind those routes: it uploads host
 * logits [n_rows][n_logits] packed (rows behind the first are 16-byte aligned only when n_logits % 4 == 0) and returns every row's id;
 * which = 0: k_argmax_advance, one launch per row (the solo loop's kernel); which = 1: one k_batch_argmax launch, one workgroup per row
 * (ticks, verify).  Both must return the same id for every row.  n_logits outside 1..65536: LH_ESHAPE; n_rows = 0, a null argument, any
 * other `which`: LH_EINVAL. */
int lh_argmax_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_rows, uint32_t n_logits, int which, uint32_t* ids_out_host);
/* Device-resident greedy decode: step i evaluates one token at position past+i; the argmax (lowest
 * index on ties, the rule above) is taken on the GPU and feeds step i+1 without a host round trip.  out_tokens[i]
 * = id produced by step i.  logits_last_host (optional) receives the final step's logits.  Past the
 * window the loop swaps context (above): one host synchronisation per (ctx - keep) / 2 tokens. */
int lh_llama_decode_greedy(lh_llama* m, uint32_t first_token, uint32_t past, uint32_t n_steps,
                           uint32_t* out_tokens, float* logits_last_host);
/* One pipeline stage of Eval for a layer-sharded model (residual stream in/out in device memory,
 * n rows of embd floats).  First stage: x_in = NULL and token ids given either on the host (tokens) or,
 * for n = 1, in device memory (tokens_dev: the id the last stage produced, received over xGMI, without
 * a host round trip).  Last stage: writes logits of the last token to logits_dev (vocab floats) and its
 * argmax to *argmax_dev (both device pointers, optional).  Asynchronous on the context's stream. */
int lh_llama_stage(lh_llama* m, const uint32_t* tokens, const uint32_t* tokens_dev, const float* x_in_dev, float* x_out_dev,
                   uint32_t n, uint32_t past, float* logits_dev, uint32_t* argmax_dev);
/* ---- sampler on the device --------------------------------------------------------------
 * SampleTopPTopK (llama.go:455-707): repeat penalty over the whole lastNTokens ring (llama.go:497-525), sort + topK
 * (llama.go:548-567), softmax with f64 exp (llama.go:581-609), topP cut (llama.go:623-639), then the reference's
 * "probs^2 * rand^2, first maximum" pick (llama.go:661-673).  The reference seeds math/rand from the clock on every
 * call (llama.go:658); here the uniforms come from a counter-based generator over (seed, call index, rank), so a
 * run is reproducible.  Ties in the sort (unspecified in the reference, sort.Slice) go to the lower token id. */
typedef struct lh_sample_params {
    uint32_t top_k;        /* ModelParams.TopK, 40 (main.go:87); 1..min(vocab, 1024) */
    float top_p;           /* 0.95 (main.go:88); >= 1 disables the cut */
    float temp;            /* > 0 (main.go:379-381 turns 0 into 0.5) */
    float repeat_penalty;  /* 1.10 (main.go:90) */
    uint64_t seed;
} lh_sample_params;
/* One call on host logits (op-level parity): last_n_tokens = the ring contents (membership only, order free).
 * cand_ids / cand_probs / n_keep (optional, top_k entries) return the kept candidates in rank order after the
 * topP rescale, i.e. the reference's logitsID / probs right before the random pick. */
int lh_sample_top_p_top_k(lh_ctx* ctx, const float* logits, uint32_t n_logits, const uint32_t* last_n_tokens, uint32_t n_last,
                          const lh_sample_params* sp, uint64_t draw, uint32_t* token_out,
                          uint32_t* cand_ids, float* cand_probs, uint32_t* n_keep);
/* The generation loop of server.Do (server.go:127-217) resident on the device: ring of ring_size zeros
 * (server.go:127-138; the reference uses CtxSize), prompt ids appended and evaluated in one Eval, then
 * n_predict x { sample -> append -> Eval(N = 1) } with no Eval after the last sample.  Sampling call s uses draw = s.
 * No host round trip per token; out_tokens gets the n_predict sampled ids. */
int lh_llama_decode_sample(lh_llama* m, const uint32_t* prompt, uint32_t n_prompt, uint32_t n_predict, uint32_t ring_size,
                           const lh_sample_params* sp, uint32_t* out_tokens);

/* ---- scoring token sequences on the device ---------------------------------------------------------------------------
 * The reference evaluates the lm_head for all N rows of an Eval (llama.go:384) and reads only the last (llama.go:394-401); its
 * softmax takes exp in f64 (llama.go:581-609, ml.go:2491).  Per row x[0..V) with target id t:
 *   m = max_j x_j;  s = sum_j exp_f64((double)x_j - (double)m) in f64;  lse = m + ln(s);  logprob = (double)x_t - lse.
 * Entries equal to -inf add 0.  A row that holds a NaN, or whose maximum is +inf or -inf, gives logprob = lse = NaN; with a NaN in
 * the row the other fields are unspecified except argmax < V. */
typedef struct lh_row_score {
    double   logprob;        /* ln p(targets[i] | row i) */
    double   lse;            /* ln sum_j exp(x_j) of the row */
    float    target_logit;   /* x[targets[i]] */
    float    max_logit;      /* x[argmax] */
    uint32_t argmax;         /* lowest index on ties: the greedy id of the generation loops */
    uint32_t target_rank;    /* number of j with x_j > x_t, plus number of j < t with x_j == x_t (0 = the target is the greedy id) */
} lh_row_score;
/* One call on host logits [n_rows][n_logits] (op-level parity, the twin of lh_sample_top_p_top_k): uploads, scores every row against
 * targets_host[row] on the device, returns after the stream drained.  targets_host[i] >= n_logits: LH_EINVAL, nothing is enqueued. */
int lh_score_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_rows, uint32_t n_logits, const uint32_t* targets_host, lh_row_score* out_host);
/* llama.Eval of tokens[0..n) at position past with the lm_head for ALL n rows (llama.go:384), every row scored on the device:
 * out_host[i] for the logits that follow tokens[i].  The [n][vocab] logits never leave the device; n * 32 bytes come back.
 * targets == NULL: the next token, targets[i] = tokens[i+1]; the last row has none and is scored against its own greedy id
 * (target_rank = 0).  The KV cache and the context's token history are left as lh_llama_eval with the same arguments leaves them.
 * Whole-model plans, weight_dtype 0, 1, 2 and 7; a stage that lacks the lm_head (or the embeddings) returns LH_EUNSUPPORTED.  past + n
 * beyond the window, a token or a target outside the vocabulary: LH_EINVAL before anything is enqueued. */
int lh_llama_score(lh_llama* m, const uint32_t* tokens, uint32_t n, uint32_t past, const uint32_t* targets, lh_row_score* out_host);

/* ---- lossless lookup-draft speculative decoding (greedy) -------------------------------------------------------------
 * Every one-token step streams all weights; a pass of 2..8 rows (block-int8: 2..4) rides the same stream with every row bit-identical to
 * its solo step.  So: draft K tokens, evaluate [pending, d1..dK] as ONE pass of the context's own cache (a causal chunk), keep the longest
 * prefix the model itself produced.  The accepted ids and their logits are the bytes lh_llama_decode_greedy produces.  Greedy only,
 * whole-model plans, weight_dtype 0, 1, 2 and 7.
 *
 * The draft rule (tests/speculative_ref.py restates it).  H[0..n) = the tokens at positions 0..n-1 of the window, H[n-1] the pending token;
 * an entry the context does not know (0xFFFFFFFF) never matches anything.  For G from ngram_max down to ngram_min: skip G when n < G or
 * when the suffix S = H[n-G..n) holds an unknown entry.  Window first: the largest j <= n-G-1 with H[j..j+G) == S gives the draft
 * H[j+G .. min(j+G+K, n)).  Else the corpus: the largest j with j+G < n_corpus and C[j..j+G) == S gives C[j+G .. min(j+G+K, n_corpus)).
 * The first G with a match wins; no match = an empty draft.  The draft ends in front of the first unknown entry of its continuation and
 * is cut to k = min(len, limit); in the loop limit = min(ctx - n, remaining - 1), remaining = n_steps - ids produced so far, so a pass
 * never leaves the window and never produces more ids than asked. */
typedef struct lh_lookup_params {
    uint32_t draft_max;            /* K: 1..7 (block-int8: 1..3; lh_batch_decode_lookup: 1..7 for both) */
    uint32_t ngram_max, ngram_min; /* 1 <= ngram_min <= ngram_max <= 8 */
    const uint32_t* corpus;        /* optional host tokens searched behind the window; NULL / 0 = none */
    uint32_t n_corpus;             /* <= 65536 */
} lh_lookup_params;
typedef struct lh_spec_stats { uint32_t passes, rows, drafted, accepted, empty; } lh_spec_stats;
/* The drafter on its own (op-level twin, host in / host out, like lh_score_rows): the rule above on window[0..n_window) with the given
 * limit; draft_out has room for draft_max ids, *n_draft = k.  No vocabulary here: only 0xFFFFFFFF is unknown. */
int lh_draft_lookup(lh_ctx* ctx, const uint32_t* window, uint32_t n_window, const lh_lookup_params* lp, uint32_t limit,
                    uint32_t* draft_out, uint32_t* n_draft);
/* One verify pass, the hook for any other drafter: tokens[0] = the pending token, tokens[1..n) a draft from anywhere, 1 <= n <= 8
 * (block-int8: 4).  ONE pass of n rows of the context's own cache at positions past..past+n-1, the lm_head for every row, per-row argmax
 * (lowest index on ties) and the accepted count a = the leading i < n-1 with argmax(row i) == tokens[i+1], all on the device.
 * ids_out[0..a] = the greedy ids of rows 0..a (room for n), *n_accepted = a, logits_host (optional, vocab floats) = row a.  Afterwards the
 * context stands at past + a + 1 and its history holds tokens[0..a] at past..past+a; the cache rows behind are stale and are overwritten by
 * whatever runs next.  Host-synchronous.  Refused before anything is enqueued: past + n > ctx, n out of range, a token id >= vocab
 * (LH_EINVAL); a layer-shard stage, a shape without an n-row pass on the decode stream (LH_EUNSUPPORTED). */
int lh_llama_verify(lh_llama* m, const uint32_t* tokens, uint32_t n, uint32_t past, uint32_t* ids_out, uint32_t* n_accepted, float* logits_host);
/* lh_llama_decode_greedy through verify passes drafted by the rule above: exactly the n_steps ids that loop produces from the same state,
 * logits_last_host byte-equal to its, the context left as it leaves it (position past + n_steps, every evaluated token in the history; a
 * context swap at the window's end as there).  Every pass has R = draft_max + 1 rows (lowered to the largest count this plan's shapes
 * carry; R = 1 = plain greedy steps), the rows behind the draft being filler that never counts.  The loop is device-resident: drafter,
 * accept step and positions live in device memory, the pass is one captured graph, and the host looks (one 64-byte read) only when its
 * bounds on the position - `passes` and `passes * R` behind the last look - reach n_steps or the window's end.
 * stats: rows = R; passes, drafted, accepted = sums over the passes; empty = passes with k = 0.  trace[s] = (k_s << 8) | a_s for
 * s < trace_cap.  Refused before anything is enqueued (context untouched): draft_max outside 1..7 (block-int8 1..3), bad n-gram bounds,
 * n_corpus > 65536, a corpus id >= vocab, first_token >= vocab, past > ctx (LH_EINVAL); a layer-shard stage (LH_EUNSUPPORTED). */
int lh_llama_decode_lookup(lh_llama* m, uint32_t first_token, uint32_t past, uint32_t n_steps, const lh_lookup_params* lp,
                           uint32_t* out_tokens, float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);

/* ---- lossless draft-model speculative decoding (greedy): a second model drafts ------------------------------------------
 * lh_llama_decode_greedy of `target` through verify passes whose drafts come from `draft`, a second whole model with a KV cache of its own on the
 * same lh_ctx: the target's own block-int8 or f16 form, another seed, a smaller geometry - anything with the same vocabulary (weight_dtype 0, 1, 2 or
 * 7).  The draft can only change how many passes are needed, never an id.  The rule (tests/draft_model_ref.py restates it):
 *   state   pos = the position of the pending token t; produced = the ids in the output list; ctx = min(target window, draft window);
 *           R = draft_len + 1, lowered to the largest row count the TARGET plan's shapes carry (as lh_llama_decode_lookup lowers it); R = 1 = plain
 *           greedy steps of the target, nothing is drafted.
 *   a pass  limit = min(ctx - (pos + 1), n_steps - produced - 1), k = min(R - 1, limit): the lookup loop's limit.
 *     draft   e_0 = t; for j = 0..k the draft model evaluates e_j at position pos + j of its own cache as a one-token step, and e_{j+1} is that
 *             step's greedy id (lowest index on ties).  The step j = k is there for the draft's cache row only, its id is not used: whatever the
 *             outcome a <= k, the draft's cache then holds the committed tokens through pos + a - no catch-up step, no condition on past.
 *     verify  the target evaluates [e_0 .. e_k] at pos .. pos + k as ONE pass of R rows (the rows behind k are filler that never counts); y_i = the
 *             greedy id of row i; a = the largest a <= k with y_i == e_{i+1} for all i < a.
 *     commit  y_0 .. y_a go to the output; pos += a + 1, t = y_a, produced += a + 1.
 *   stats and trace as lh_llama_decode_lookup: drafted += k, accepted += a, empty counts the passes with k = 0, trace[s] = (k_s << 8) | a_s.
 * The pass is device-resident: k_draft_model_begin (the draft's step parameters, k, filler), R one-token steps of the draft (each id straight
 * into the target's token table), the target's R-row pass, k_batch_argmax, k_spec_accept - all enqueued on the context's stream with no host
 * round trip inside a pass or between passes.  The launches of a pass are enqueued kernel by kernel; they are not replayed from a captured graph
 * (DESIGN 3i says why).  Near the window's end, where ctx - pos < R, narrower passes run; a pass that would stand outside the window is never
 * enqueued, and should one be, k_draft_model_begin ends the loop in the device state and the call fails (LH_EHIP).  The host looks (one 64-byte
 * read) where the lookup loop looks.
 * Precondition (the library cannot check it): both caches hold the same tokens at [0, past).
 * Afterwards: out_tokens = exactly the n_steps ids of lh_llama_decode_greedy(target, ...) from the same state, logits_last_host byte-equal to its;
 * the target stands as that loop leaves it (position past + n_steps, every evaluated token in its history, usable by lh_llama_decode_lookup); the
 * draft holds valid rows and history for [0, past + n_steps) (with R = 1 through one Eval of the evaluated tokens behind the steps); rows behind
 * that are stale in both caches.  No context swap here: the window bound replaces it.
 * Refused before anything is enqueued, both contexts untouched and usable: draft == target, different lh_ctx, different vocabularies, draft_len
 * outside 1..7 (block-int8 target: 1..3), first_token >= vocab, past + n_steps > ctx (LH_EINVAL); a layer-shard stage on either side
 * (LH_EUNSUPPORTED). */
int lh_llama_decode_draft(lh_llama* target, lh_llama* draft, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t draft_len,
                          uint32_t* out_tokens, float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap);

/* ---- lossless lookup-draft speculative decoding (sampled) ------------------------------------------------------------
 * The uniforms of the device sampler are counter-based (seed, sampling call, rank), so the id of sampling call s is a pure function of the
 * logits row, the lastNTokens ring at that moment and s.  A pass over [pending, d1..dk] therefore samples every row at once, and the kept ids
 * are EXACTLY those of lh_llama_decode_sample - an equality, no rejection sampling.  The rule, with the sampler state {ring, ring_pos = ids
 * appended so far (next slot = ring_pos % ring_size), draw = index of the next sampling call} in front of the pass:
 *   ring view of row r: the ring after tok[1..r] were appended in order, ring[(ring_pos + j) % ring_size] = tok[j+1] for j = 0..r-1 (a slot
 *                        may be overwritten more than once when ring_size < r); the ring itself is not written by the sampler;
 *   draw of row r:       draw + r;  id of row r -> arg[r];
 *   commit:              a = the leading i < min(k, R - 1) with arg[i] == tok[i+1] (clipped by the ids still asked for and by the window);
 *                        arg[0..a] are appended to the ring in order, ring_pos += a + 1, draw += a + 1.
 * lh_sample_rows is the op-level twin of the multi-row sampler kernels (k_sample_rows, topK <= 1024; k_sample_small_rows, topK <= 64), like
 * lh_argmax_rows / lh_score_rows: host logits [n_rows][n_logits] packed, ring_host[0..ring_size) with ring_pos, tokens_host[0] ignored (the
 * pending token is in the ring already), tokens_host[1..n_rows) the draft; ONE launch, ids_out[r] = the id of row r as sampling call
 * draw0 + r.  Refused with nothing enqueued: n_rows outside 1..8, ring_size == 0, a draft id >= n_logits, bad sampler parameters, a null
 * argument (LH_EINVAL); n_logits outside 1..65536 (LH_ESHAPE); topK above 1024 (LH_EUNSUPPORTED). */
int lh_sample_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_rows, uint32_t n_logits, const uint32_t* ring_host, uint32_t ring_size,
                   uint32_t ring_pos, const uint32_t* tokens_host, const lh_sample_params* sp, uint64_t draw0, uint32_t* ids_out);
/* lh_sample_pods is the op-level twin of the multi-pod sampler kernels (k_sample_pods, topK <= 1024; k_sample_small_pods, topK <= 64): what a sampled
 * tick of an lh_batch runs.  Host logits [n][n_logits] packed, rings_host [n][ring_size] with ring_pos[i] ids appended to pod i's ring so far, draws[i] =
 * the index of pod i's sampling call, one set of parameters; ONE launch, one workgroup per pod.  ids_out[i] = SampleTopPTopK of row i over ring i as call
 * draws[i]; rings_out [n][ring_size] / ring_pos_out [n] (both optional) = the rings with that id appended.  Refusals as lh_sample_rows, with n outside
 * 1..64 in place of the row count. */
int lh_sample_pods(lh_ctx* ctx, const float* logits_host, uint32_t n, uint32_t n_logits, const uint32_t* rings_host, uint32_t ring_size,
                   const uint32_t* ring_pos, const uint64_t* draws, const lh_sample_params* sp, uint32_t* ids_out, uint32_t* rings_out,
                   uint32_t* ring_pos_out);
/* lh_llama_decode_sample through verify passes drafted by the lookup rule above: the same ring, prompt Eval and first sample on the last
 * prompt row, then the n_predict - 1 remaining ids from passes of R = draft_max + 1 rows (lowered as in lh_llama_decode_lookup; R = 1 = plain
 * sampled steps) that sample every row and commit by the rule above.  out_tokens = exactly the n_predict ids of lh_llama_decode_sample with
 * the same arguments, and the context is left as that call leaves it (position, history, ring, draw counter, context swaps).  stats / trace
 * as lh_llama_decode_lookup, over the passes behind the first sample.  Refused before anything is enqueued: everything lh_llama_decode_sample
 * and lh_llama_decode_lookup refuse (LH_EINVAL); a layer-shard stage (LH_EUNSUPPORTED). */
int lh_llama_decode_sample_lookup(lh_llama* m, const uint32_t* prompt, uint32_t n_prompt, uint32_t n_predict, uint32_t ring_size,
                                  const lh_sample_params* sp, const lh_lookup_params* lp, uint32_t* out_tokens, lh_spec_stats* stats,
                                  uint16_t* trace, uint32_t trace_cap);

/* ---- pods in ONE weight pass (batched decode) ---------------------------------------------------------------------
 * The reference's only parallelism is request-level: Engine() starts up to MaxPods concurrent Do() goroutines
 * (pkg/server/server.go:84-106), each with its own llama.Context over the shared Model (server.go:151).  On the CPU they share
 * the cores.  On the GPU every N = 1 Eval streams all weights, so P pods decoding on their own read P x 26.4 GB per round of
 * tokens for the bandwidth of one.  An lh_batch binds the stages of P streams (lh_llama_create with the SAME weights and layer
 * range and ONE KV cache each, all on one lh_ctx) and evaluates a decode step of all of them as one P-row pass: weights read
 * once, RoPE / cache append / attention per row at the row's own position of its own cache.  A row's result does not depend on
 * its index or on the other rows.  Shapes the P-row kernels are not built for run row by row (same results, P passes):
 * lh_batch_batched() tells.  1 <= P <= 64.  The pods must outlive the batch; while it exists use them only through it or for
 * whole-prompt Evals (lh_llama_stage / lh_llama_eval with n > 1 rows).
 * Token ids, positions and residual rows of a tick live at fixed device addresses and the tick is ONE captured hipGraph that
 * also moves the positions on: a tick costs the host one graph launch whatever the stage's length. */
typedef struct lh_batch lh_batch;
int lh_batch_create(lh_ctx* ctx, lh_llama* const* pods, uint32_t n_pods, lh_batch** out);
void lh_batch_destroy(lh_batch* b);
uint32_t lh_batch_rows(const lh_batch* b);
int lh_batch_batched(const lh_batch* b);          /* 1: the rows share one weight pass; 0: row by row */
/* Device arrays a transport delivers into / reads from: [rows] ids evaluated by the next tick (first stage) and [rows] ids the
 * last tick produced (last stage).  On a whole-model batch a tick feeds the second into the first itself. */
uint32_t* lh_batch_tokens_dev(lh_batch* b);
uint32_t* lh_batch_ids_dev(lh_batch* b);
int lh_batch_read_ids(lh_batch* b, uint32_t* ids_host);   /* waits for the stream, then copies the [rows] produced ids to the host */
/* Position (= llama.Eval's pastCount) of every row's next token and, tokens != NULL, the ids themselves (first stage), from the
 * host; the rows' output lists restart. */
int lh_batch_set(lh_batch* b, const uint32_t* tokens_or_null, const uint32_t* past);
/* server.Do's prompt Eval (server.go:185-192) for every row, each on its own cache at position 0: prompts[i][0..n_prompt[i])
 * (host; first stage only, n_prompt on every stage).  Later stages read / earlier stages write the rows of all prompts one after
 * the other in x_in_dev / x_out_dev (sum(n_prompt) x embd floats).  The last stage leaves each row's next id (argmax of its last
 * prompt row, or the first sampler draw) in lh_batch_ids_dev; every stage then stands at position n_prompt[i] per row. */
int lh_batch_prompt(lh_batch* b, const uint32_t* const* prompts, const uint32_t* n_prompt, const float* x_in_dev, float* x_out_dev);
/* One decode tick for every row (llama.Eval with N = 1 per stream, llama.go:211-426): x_in_dev / x_out_dev = [rows][embd]
 * residual rows from the previous / for the next stage (NULL on the first / last stage).  Optional device copies of the
 * [rows][vocab] logits and the [rows] produced ids.  Asynchronous on the context's stream; positions advance by one. */
int lh_batch_stage(lh_batch* b, const float* x_in_dev, float* x_out_dev, float* logits_dev, uint32_t* ids_dev);
/* From now on the last stage draws every row's id with SampleTopPTopK (llama.go:455-707; same device sampler and counter-based
 * uniforms as lh_llama_decode_sample, every row seeded like a solo run) instead of the argmax.  ring_init[i][0..n_init[i]) = ids
 * already appended to row i's lastNTokens ring of ring_size slots (the prompt, server.go:193-197).  sp = NULL: back to greedy. */
/* A sampled tick is ONE sampler launch over all rows (k_sample_pods / k_sample_small_pods, one workgroup per row); LLAMAHIP_SAMPLE_PER_POD=1 (debug / A-B,
 * read when the tick is captured) keeps one launch per row - ids, rings and draw counters are the same either way. */
int lh_batch_set_sampler(lh_batch* b, const lh_sample_params* sp, uint32_t ring_size, const uint32_t* const* ring_init, const uint32_t* n_init);
/* Whole-model pods: n_steps device-resident ticks from (first_tokens[i], past[i]); out_tokens[i * n_steps + s] = id row i
 * produced at step s; logits_last_host (optional) = [rows][vocab] logits of the final tick.
 * Context swap: a tick (here and in lh_batch_stage) of a WHOLE-MODEL batch whose row stands at the window's end first swaps that row's
 * context as server.Do does (server.go:160-172, lh_llama_set_keep per pod): the re-fed run is evaluated as one Eval on the row's own
 * cache, then the tick takes the row's pending token behind it.  It needs the tokens of the row's window, which the batch knows when the
 * row's prompt ran through lh_batch_prompt (or its Evals through its lh_llama with host ids); otherwise, and for a stage of a layer shard,
 * such a tick fails with LH_EINVAL before anything is enqueued. */
int lh_batch_decode(lh_batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, uint32_t* out_tokens, float* logits_last_host);
/* lh_batch_decode through lookup-drafted verify passes (the draft rule of lh_lookup_params, per pod over the pod's own window; ONE corpus for all pods):
 * speculation and the shared weight stream at once.  Greedy only, whole-model batches, weight_dtype 0, 1, 2 and 7.  With P = the number of pods, every pass has
 * P * R rows: row i * R + r is row r of pod i, on pod i's cache at position pos_i + r, holding [pending_i, d_1..d_k, filler = pending_i] - the order in
 * which lh_batch_feed lays out P pods fed R tokens each.  R = draft_max + 1, lowered to the largest R with P * R <= 64 whose row count shares one weight
 * pass on this plan (the predicate behind the feed's sizes_ok); a batch of two or more pods that is not lh_batch_batched takes R = 1.  R = 1 = plain
 * ticks (the lh_batch_decode route); stats[i].rows reports R.  draft_max is 1..7 for both weight types.
 * Per pod and pass: limit = min(ctx - n, remaining_i - 1); a = the leading i < k with argmax(row i) == tok[i + 1] (fillers never count), clipped by what
 * the pod still needs; ids arg[0..a] go to its output list and window.  A pod with n_steps ids is finished: its rows stay in the pass as filler (they
 * re-evaluate the tokens of its finishing pass at their positions) and its state, output list and window no longer change.  Every pass gives every
 * unfinished pod 1..R ids, so the host enqueues ceil((n_steps - min_i produced_i) / R) passes - one captured graph: the batched Eval, k_batch_argmax,
 * k_spec_accept_pods - reads 16 bytes per pod and repeats; it never enqueues a pass that could find every pod finished.
 * The loop never leaves the window and never swaps context: past[i] + n_steps + R - 1 <= ctx must hold for every pod (LH_EINVAL otherwise), so no row
 * of any pass stands past the window; the caller takes the last R - 1 positions with ticks.
 * Contract:
 *  1. the rows of a pass are byte-equal to the rows lh_batch_feed computes for the same tokens and positions with LLAMAHIP_FEED_ROW_ATTN=1 (the same
 *     launch sequence);
 *  2. where P * R <= 8 (fp32) or <= 4 (block-int8) the ids equal lh_batch_decode's and each pod's solo lh_llama_decode_greedy, and for fp32
 *     logits_last_host is byte-equal too (the bit-identity of the rows path);
 *  3. beyond, the ids are the greedy ids of the passes' own logits, at the tolerance of ticks of more than 8 pods.  No more is claimed.
 * out_tokens [rows][n_steps] as lh_batch_decode; logits_last_host (optional) [rows][vocab] = the logits behind each pod's LAST id (row a of its finishing
 * pass); stats (optional) [rows]; trace (optional) [rows][trace_cap]: (k << 8) | a per pass of that pod.
 * Afterwards the batch stands as lh_batch_decode(first_tokens, past, n_steps) leaves it: positions past + n_steps (host mirror included), each pod's last
 * id pending in lh_batch_tokens_dev, lh_batch_ids_dev and entry 0 of its output list (lh_batch_feed's conventions), every evaluated token in the pods'
 * histories; cache rows behind each position are stale and are overwritten by whatever runs next.
 * Refused before anything is enqueued, the batch left exactly as it was: the window condition, bad lookup parameters, a corpus id or first token >= vocab,
 * n_steps == 0, a null required argument (LH_EINVAL); a batch with a sampler set, a batch of layer-shard stages (LH_EUNSUPPORTED).
 * A batch with a sampler set takes lh_batch_decode_sample_lookup (below).
 * Out of scope: a context swap or shrinking passes at the window's end, segment attention for the pass, per-pod n_steps or corpora. */
int lh_batch_decode_lookup(lh_batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp,
                           uint32_t* out_tokens,        /* [rows][n_steps], as lh_batch_decode */
                           float* logits_last_host,     /* optional [rows][vocab] */
                           lh_spec_stats* stats,        /* optional [rows] */
                           uint16_t* trace,             /* optional [rows][trace_cap] */
                           uint32_t trace_cap);
/* The accept step of such a pass on its own (op-level twin of k_spec_accept_pods, host in / host out like lh_draft_lookup): arg [n_pods][n_rows] = the
 * greedy ids of the pass's rows, tok [n_pods][n_rows] = the tokens they evaluated, k[i] = pod i's draft length, pos[i] / produced[i] its state in front
 * of the pass.  ONE launch, no drafting.  a_out[i] = the accepted count, pos_out / produced_out / pending_out the state behind the pass, ids_out
 * [n_pods][n_rows] = the ids appended to pod i's list (entries behind them 0xFFFFFFFF).  A finished pod (produced[i] >= n_steps) comes back unchanged.
 * n_pods outside 1..64, n_rows outside 1..8, n_pods * n_rows > 64, ctx_size == 0, a null argument: LH_EINVAL. */
int lh_spec_accept_pods(lh_ctx* ctx, const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos,
                        const uint32_t* produced, uint32_t n_steps, uint32_t ctx_size, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out,
                        uint32_t* pending_out, uint32_t* ids_out);
/* ---- the same for a SAMPLING batch: the loop a server with sampling on runs (server.go:201-217 per pod, TopK 40; the pods side by side, server.go:84-106).
 * lh_batch_decode_sample_lookup is lh_batch_decode_lookup on a batch behind lh_batch_set_sampler, with two launches exchanged: ONE sampler launch over the
 * P * R rows of the pass (k_sample_pod_rows, topK <= 1024; k_sample_small_pod_rows, topK <= 64) in place of the argmax, and the accept step commits every
 * pod's ring and draw counter.  The rule per pod i is the rule of lh_llama_decode_sample_lookup on the pod's own sampler state: row r of pod i is
 * SampleTopPTopK (llama.go:455-707) of logits row i * R + r as sampling call draw_i + r over pod i's ring as if tok[i * R + 1 .. i * R + r] had been appended
 * behind its ring_pos ids; a = the leading j < k_i with arg[j] == tok[j + 1] (clipped as above); arg[0..a] are appended to pod i's ring in order
 * (appendToken, server.go:205), ring_pos_i and draw_i move on by a + 1.  The uniforms are counter-based (seed, sampling call, rank), so this is an equality
 * with the one-token ticks, no rejection sampling.  R (batch_spec_rows), the window condition past[i] + n_steps + R - 1 <= ctx, the host's look cadence, one
 * captured graph per pass (re-captured also when the sampler variant, the ring or the state array changed), R = 1 = plain sampled ticks (the lh_batch_decode
 * route), stats and trace: all as lh_batch_decode_lookup.
 * Contract:
 *  1. out_tokens = the ids of lh_batch_decode on the same sampling batch from the same state with the same arguments; so where P * R <= 8 (fp32) or <= 4
 *     (block-int8) they are also each pod's solo lh_llama_decode_sample ids;
 *  2. for any row count they are the sampler's ids on the pass's own logits (rows byte-equal to lh_batch_feed's with LLAMAHIP_FEED_ROW_ATTN=1);
 *  3. afterwards the batch stands as lh_batch_decode leaves it: positions past + n_steps (host mirror included), each pod's last id pending in
 *     lh_batch_tokens_dev, lh_batch_ids_dev and entry 0 of its output list, every pod's ring, ring_pos and draw equal to what the ticks would hold, the
 *     evaluated tokens in the pods' histories.
 * logits_last_host (optional) [rows][vocab] = the row each pod's LAST id was sampled from.
 * Refused before anything is enqueued, batch and sampler state left exactly as they were: everything lh_batch_decode_lookup refuses; a batch without a
 * sampler (LH_EINVAL, as lh_batch_feed_sample); a batch of layer-shard stages (LH_EUNSUPPORTED).
 * Out of scope: a context swap or shrinking passes at the window's end, segment or shared-prefix attention for the pass, per-pod seeds, parameters, n_steps
 * or corpora, layer shards and the pipeline. */
int lh_batch_decode_sample_lookup(lh_batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp,
                                  uint32_t* out_tokens,        /* [rows][n_steps], as lh_batch_decode */
                                  float* logits_last_host,     /* optional [rows][vocab] */
                                  lh_spec_stats* stats,        /* optional [rows] */
                                  uint16_t* trace,             /* optional [rows][trace_cap] */
                                  uint32_t trace_cap);
/* The sampler launch of such a pass on its own (op-level twin of k_sample_pod_rows / k_sample_small_pod_rows, host in / host out like lh_sample_rows and
 * lh_sample_pods): SampleTopPTopK (llama.go:455-707) for the rows of n_pods generation loops (server.go:201-217) at once.  logits_host [n_pods * n_rows]
 * [n_logits] packed, rings_host [n_pods][ring_size] with ring_pos[i] ids appended so far, draws[i] = pod i's next sampling call, tokens_host [n_pods][n_rows]
 * (entry 0 of a pod, its pending token, is ignored: it is in the ring already), n_draft[i] = pod i's draft length, one set of parameters.  ONE launch.
 * ids_out[i * n_rows + r] = the id of row r of pod i for r <= n_draft[i]; the other entries are not written (the caller presets 0xFFFFFFFF).  Refusals as
 * lh_sample_rows, with n_pods outside 1..64, n_rows outside 1..8 or n_pods * n_rows > 64 in place of the row count. */
int lh_sample_pod_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_pods, uint32_t n_rows, uint32_t n_logits, const uint32_t* rings_host,
                       uint32_t ring_size, const uint32_t* ring_pos, const uint64_t* draws, const uint32_t* tokens_host, const uint32_t* n_draft,
                       const lh_sample_params* sp, uint32_t* ids_out);
/* lh_spec_accept_pods with the sampled commit (k_spec_accept_pods on the sampled route): additionally rings [n_pods][ring_size], ring_pos [n_pods] and
 * draws [n_pods] in front of the pass; rings_out / ring_pos_out / draws_out (each optional) behind it - a pod that accepts a has arg[0..a] appended to its
 * ring in order (appendToken, server.go:205, once per id of the loop server.go:201-217) and both counters moved on by a + 1; a finished pod commits nothing.
 * ONE launch.  Refusals as lh_spec_accept_pods, and ring_size == 0 or a null ring argument (LH_EINVAL). */
int lh_spec_accept_sample_pods(lh_ctx* ctx, const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos,
                               const uint32_t* produced, uint32_t n_steps, uint32_t ctx_size, const uint32_t* rings, uint32_t ring_size,
                               const uint32_t* ring_pos, const uint64_t* draws, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out,
                               uint32_t* pending_out, uint32_t* ids_out, uint32_t* rings_out, uint32_t* ring_pos_out, uint64_t* draws_out);
/* Pod `pod`'s sampler state of a sampling batch, after waiting for the stream: its lastNTokens ring (server.go:127-138; ring_out has room for
 * lh_batch_sampler_ring_size(b) ids: the ring_size of the last lh_batch_set_sampler, 0 for a batch without a sampler), ring_pos = ids appended so far and draw = the index of its next sampling call (llama.go:658 seeds per call).  Each output is
 * optional.  A batch without a sampler, a pod outside the batch: LH_EINVAL. */
uint32_t lh_batch_sampler_ring_size(const lh_batch* b);
int lh_batch_sampler_read(lh_batch* b, uint32_t pod, uint32_t* ring_out, uint32_t* ring_pos_out, uint64_t* draw_out);
/* llama.Eval for any subset of the pods, packed into shared weight passes of <= 64 rows (whole-model batches, greedy).
 * Pod i evaluates tokens[i][0..n_tokens[i]) at positions past[i].. of ITS cache.
 * n_tokens[i] == 0: pod i is not fed (tokens[i], past[i] ignored).
 * A fed pod afterwards stands at past[i] + n_tokens[i]; its next tick evaluates the greedy id of its last fed row (in lh_batch_ids_dev, in
 * lh_batch_tokens_dev and in entry 0 of the row's output list - the conventions lh_batch_prompt leaves); its tokens are in the pod's window
 * history, so a later context swap knows them; a pending id it had before the feed is dropped (feed it to have it evaluated).
 * A pod that is not fed keeps its position, the token its next tick evaluates, its KV cache and what a context swap knows of it.  The output
 * lists of ALL rows restart (as with lh_batch_set).  The first feed of a fresh batch (no lh_batch_set / lh_batch_prompt yet) must feed every row.
 * c consecutive rows of one pod in a pass are a causal prompt chunk: the wq|wk|wv launch appends every row's K / V before the attention launch
 * reads them.  Which rows share which pass is lh_feed_schedule's fixed partition (below), so results never depend on timing.
 * Refused before anything is enqueued, the batch left exactly as it was: past[i] + n_tokens[i] > ctx, a token id >= vocab, all n_tokens[i] == 0,
 * tokens[i] == NULL with n_tokens[i] > 0 (LH_EINVAL); a batch with a sampler set, a batch of layer-shard stages (LH_EUNSUPPORTED).
 * Out of scope: sampler rings across a feed (lh_batch_feed_sample below); layer shards and the pipeline; a context swap INSIDE a feed (a feed never leaves the window: the
 * swap happens in the ticks behind it); lh_batch_prompt keeps its own route (one Eval per pod).
 * Switches (read per call): LLAMAHIP_FEED_SOLO_MIN (rows from which a pod's feed is an Eval of its own, default 129), LLAMAHIP_FEED_QB (query rows
 * per attention block: 2, 4 or 8), LLAMAHIP_FEED_ROW_ATTN=1 (debug / A-B: the per-row attention kernels on the pass's row table). */
int lh_batch_feed(lh_batch* b, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past,
                  uint32_t* ids_host,          /* optional [rows]: greedy id of each FED pod's last row; other entries not written */
                  float* logits_last_host,     /* optional [rows][vocab]: logits of each fed pod's last row; other rows not written */
                  float* logits_rows_host);    /* optional [sum n_tokens][vocab]: every fed row, pods in index order */
/* lh_batch_feed on a batch whose ticks SAMPLE (lh_batch_set_sampler): jobs join and leave a running sampled batch as server.Do takes them
 * (pkg/server/server.go:127-217).  Schedule, passes, caches, histories, positions and output-list conventions are lh_batch_feed's; what differs is
 * the id behind a fed pod's last row and the pod's sampler state {ring, ring_pos, draw}.  The rule, for a fed pod i (tests/feed_sample_ref.py restates it):
 *   1. flags[i] & LH_FEED_NEW: a new job (server.go:127-138) - the ring becomes ring_size zeros, ring_pos = 0, draw = 0; seed and parameters stay the batch's;
 *   2. its fed tokens are appended to the ring in order (server.go:189-190).  With LH_FEED_PENDING the first one is NOT appended: tokens[i][0] is then
 *      the pod's pending id, which its last sampling call appended already.  It requires past[i] == the pod's position and tokens[i][0] == its pending id,
 *      both known to the host once the stream has been waited for: a feed with a PENDING flag therefore waits for the stream and reads what the ticks so
 *      far produced BEFORE it is checked (a refused one has done that much, and nothing else); otherwise the call returns LH_EINVAL;
 *   3. its last fed row is sampled as call `draw` over that ring; the id is appended, ring_pos and draw move on by one.  The id is the pod's pending
 *      token: lh_batch_ids_dev, lh_batch_tokens_dev, entry 0 of its output list and ids_host[i];
 *   4. a pod that is not fed keeps its ring, counters, pending token and cache.
 * Every feed of a pod ends in exactly ONE sampling call, so a prompt must arrive in ONE feed to draw what lh_llama_decode_sample draws for it: NEW + the
 * prompt, then ticks, makes the same sampler calls over the same ring.  Where the rows of the pass are bit-identical to solo rows (up to 8 rows per pass
 * for fp32, 4 for block-int8) the ids are equal; beyond, they are the sampler's on logits within the feed's tolerance.
 * Per pass: one k_feed_ring launch over its segments, one k_sample_pods / k_sample_small_pods launch over the segments that end in it.
 * Refused before anything is enqueued, the batch - sampler state included - left as it was: everything lh_batch_feed refuses except a set sampler; no
 * sampler set (LH_EINVAL: use lh_batch_feed); an unknown flag bit; NEW | PENDING together; a failed PENDING check (LH_EINVAL).
 * Out of scope: chunked prompts on a sampling batch, per-job seeds, layer shards. */
enum { LH_FEED_NEW = 1, LH_FEED_PENDING = 2 };
int lh_batch_feed_sample(lh_batch* b, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past,
                         const uint32_t* flags,       /* [rows] or NULL = all 0 */
                         uint32_t* ids_host,          /* optional [rows]: sampled id of each FED pod; other entries not written */
                         float* logits_last_host,     /* optional [rows][vocab]: logits of each fed pod's last row; other rows not written */
                         float* logits_rows_host);    /* optional [sum n_tokens][vocab]: every fed row, pods in index order */
/* The pass schedule of a feed: the pure function (no GPU) lh_batch_feed executes.  A pod with n_tokens >= solo_min is a solo pass (an Eval on
 * its own plan); the other fed rows, in pod order with ascending positions, are cut into batched passes of <= 64 rows (a pod's rows in a pass
 * are one segment; a segment may continue in the next pass); a pass of one row, and the segments of a pass whose row count n has bit n - 1 of
 * sizes_ok clear, are solo passes.  Blocks: <= qb consecutive rows of ONE segment of a batched pass (the query blocks of its attention).
 * Fills up to the given capacities, writes the full counts {passes, segments, blocks} to counts[3] and returns the pass count (-1: bad arguments). */
enum { LH_FEED_BATCHED = 0, LH_FEED_SOLO = 1 };
typedef struct lh_feed_pass { uint32_t kind, seg0, nseg, blk0, nblk, rows; } lh_feed_pass;   /* segments [seg0, seg0 + nseg), blocks [blk0, blk0 + nblk) */
typedef struct lh_feed_seg { uint32_t pod, row0, n, pos0; } lh_feed_seg;                      /* rows [row0, row0 + n) of its pass: pod's positions pos0.. */
typedef struct lh_feed_block { uint32_t row0, n; } lh_feed_block;                            /* rows [row0, row0 + n) of its pass */
int lh_feed_schedule(const uint32_t* n_tokens, const uint32_t* past, uint32_t rows, uint32_t solo_min, uint32_t qb, uint64_t sizes_ok,
                     lh_feed_pass* passes, uint32_t pass_cap, lh_feed_seg* segs, uint32_t seg_cap, lh_feed_block* blocks, uint32_t block_cap, uint32_t* counts);

/* ---- a common prompt prefix shared by pods of a batch ---------------------------------------------------------------
 * The pods of a server usually stand behind one identical prefix (a system prompt in front of every job, several continuations of one prompt).
 * lh_batch_fork gives pods the prefix another pod has evaluated, and the ticks then read the prefix's keys and values ONCE per block of member rows
 * instead of once per row.
 * The rule.  In stream order, cache rows [0, n_pos) of every layer slot, K and V, of pod src are copied into every pod of dst[0..n_dst) (device to
 * device; every member keeps a full copy of its own), and entries [0, n_pos) of the source's token history into the destinations' histories, so that
 * a later context swap knows them.  Nothing else moves: positions, pending tokens, output lists, sampler rings and draw counters of all pods stay as
 * they are (a fork is allowed on a sampling batch).  The caller then feeds each destination at past = n_pos (lh_batch_feed / lh_batch_feed_sample) or
 * places it with lh_batch_set.
 * Sharing groups.  The fork records {src} + dst as a group of shared length n_pos.  A pod is in at most one group.  If src already stands in a group of
 * exactly that length the destinations join it; otherwise src and the destinations leave whatever groups they were in and form a new one.  The
 * invariant of a member is "my cache rows [0, len) are byte-equal to every other member's"; ONE predicate keeps it: a pod leaves its group when
 * anything writes its cache below len - lh_batch_feed / lh_batch_feed_sample with past[i] < len, lh_batch_prompt, a tick or lh_batch_set that places it
 * at a position < len, lh_batch_decode_lookup with past[i] < len, the re-fed Eval of a context swap, anything that evaluates a token below len on the
 * pod's own lh_llama (lh_llama_eval, lh_llama_stage, lh_llama_score, the one-token step and the resident greedy, sampled, lookup and verify loops;
 * seen when the batch next looks), and whoever writes the cache from outside says so with lh_batch_share_written.  A group of one member dissolves.
 * A fork first reads the ids of the ticks so far into the pods' histories (a stream wait, only if there are such ticks), so that no later read
 * records a destination's old tokens over the history it was given.
 * Ticks.  Where the batch shares one weight pass and its plan has split attention partials (ctx > 256, head size 128) a tick runs
 * k_attention_split_shared on k_attention_split's grid: the full 128-key chunks inside a group's prefix are loaded once per block of member rows (the
 * blocks: lh_share_schedule below) from the block's first row's OWN cache, every other chunk and every row without a block as before, the partial
 * records in the same slots, k_attention_combine unchanged.  Per query row the operations and their order are k_attention_split's, so every logit of
 * every tick is byte-equal to the per-row kernels' (LLAMAHIP_SHARE_ROW_ATTN=1 keeps those: the A/B switch).  Elsewhere a fork still copies and ticks
 * run as before.  Feeds, lh_batch_decode_lookup passes and prompt Evals keep their own attention routes.
 * State left behind: the destinations' cache rows [0, n_pos) and histories as the source's; rows >= n_pos of every cache untouched; the group state.
 * Refused before anything is enqueued, the batch left exactly as it was: src or a dst[i] outside the batch, dst naming src or a pod twice, n_dst == 0,
 * n_pos == 0, n_pos beyond the source's position in the host mirror or the mirror not placed yet (LH_EINVAL); a batch of layer-shard stages
 * (LH_EUNSUPPORTED).
 * Out of scope: freeing or never allocating the members' own copies (copy-on-write), shared reads in feeds, in lookup passes and in the single-pass
 * k_attention (ctx <= 256), layer shards and the pipeline, per-pod sampler seeds, detecting equal prefixes by itself.
 * Switches (read per tick; a change that alters the tick's launches re-captures it): LLAMAHIP_SHARE_ROW_ATTN=1, LLAMAHIP_SHARE_QB = 2 | 4 | 8 (rows
 * per block), LLAMAHIP_SHARE_MIN (smallest group that gets blocks). */
int lh_batch_fork(lh_batch* b, uint32_t src, const uint32_t* dst, uint32_t n_dst, uint32_t n_pos);
/* Per pod the lowest pod index of its sharing group and the shared length; a pod that shares nothing: its own index and 0.  Host state only (no
 * stream wait).  Both arrays [rows]. */
int lh_batch_share_info(lh_batch* b, uint32_t* group_out, uint32_t* len_out);
/* The leave rule for writers the batch cannot see (a host upload into a pod's cache): something wrote pod's cache rows from position pos_lo on.  The
 * pod leaves its group if pos_lo lies below the shared length.  Host state only.  pod outside the batch: LH_EINVAL. */
int lh_batch_share_written(lh_batch* b, uint32_t pod, uint32_t pos_lo);
/* The block table of a tick: the pure function (no GPU) the tick executes.  group / len [rows] as lh_batch_share_info returns them.  Groups in
 * ascending order of their lowest member, members ascending, cut into blocks of at most qb rows (2, 4 or 8); chunks = len / 128 full key chunks lie
 * inside the prefix; a group with chunks == 0 or fewer than min_rows members, and a trailing block of one row, get no block.  row_block[j] (optional,
 * [rows]) = the block of row j or 0xFFFFFFFF.  blocks == NULL: the sizing call.  Returns the block count; -1: a null group / len, rows outside 1..64,
 * another qb, a group index that is not its group's lowest member, members of one group with different lengths, cap below the count (nothing written). */
typedef struct lh_share_block { uint32_t n, chunks, row[8]; } lh_share_block;   /* rows row[0..n) share the first `chunks` key chunks */
int lh_share_schedule(const uint32_t* group, const uint32_t* len, uint32_t rows, uint32_t qb, uint32_t min_rows, lh_share_block* blocks, uint32_t cap,
                      uint32_t* row_block);

/* ---- multi-GPU: layer shard over RCCL point-to-point ------------------------------------------------
 * The reference's only parallel dimension is request-level "pods" (pkg/server/server.go:84-106: Engine() starts up to
 * MaxPods concurrent Do() goroutines; server.go:151: each with its own llama.Context over the shared Model).  Layers
 * shard in contiguous blocks over one process per GPU; the fp32 residual stream [n x embd] hops rank r -> r+1 and the
 * sampled token id returns from the last rank to rank 0, both as RCCL send/recv over xGMI, issued HERE (on the context's
 * stream, grouped) so that a Go host needs no collective library of its own: it only moves the 128-byte unique id from
 * rank 0 to the other ranks over whatever channel it already has (a file, a socket, its job queue).
 * librccl.so.1 is loaded on first use (dlopen), so single-GPU hosts never need it. */
#define LH_COMM_ID_BYTES 128
typedef struct lh_comm lh_comm;
int lh_comm_unique_id(lh_ctx* ctx, uint8_t id[LH_COMM_ID_BYTES]);       /* ncclGetUniqueId: call on rank 0, distribute */
int lh_comm_init(lh_ctx* ctx, int rank, int world, const uint8_t id[LH_COMM_ID_BYTES], lh_comm** out); /* ncclCommInitRank on ctx's device */
/* Alternative transport for hosts without RCCL peers (tests with several ranks on ONE GPU, which RCCL refuses; TCP):
 * the library stages the messages through host memory and hands both directions of a tick to ONE call, which must
 * post the send and the receive together (a ring of blocking sends would wait on itself).  NULL buffers = no message. */
/* ABI note: lh_comm_init_hooks copies the WHOLE struct and lh_comm_abort calls `abort` whenever it is non-NULL: zero-initialise the struct
 * (`lh_comm_hooks h = {0};`) and set the members you provide - a host that fills only `user` / `exchange` of an uninitialised struct
 * hands the library an indeterminate function pointer.  The struct's size is part of ABI version 1 (lh_abi_version). */
typedef struct lh_comm_hooks {
    void* user;
    int (*exchange)(void* user, const void* send_host, uint64_t send_bytes, int send_peer, void* recv_host, uint64_t recv_bytes, int recv_peer);
    /* optional (may be NULL): lh_comm_abort on this transport - make what the PEERS have pending against this rank fail instead of
     * block (the counterpart of ncclCommAbort: e.g. send them a message of the wrong size, or close the connection) */
    void (*abort)(void* user);
} lh_comm_hooks;
int lh_comm_init_hooks(lh_ctx* ctx, int rank, int world, const lh_comm_hooks* hooks, lh_comm** out);
void lh_comm_destroy(lh_comm* comm);
/* Tear the communicator down without waiting for the peers (ncclCommAbort): what they have pending against this rank fails instead
 * of blocking.  Used by lh_pipeline_run when a rank fails mid-run; afterwards only lh_comm_destroy is valid. */
int lh_comm_abort(lh_comm* comm);
int lh_comm_rank(const lh_comm* comm);
int lh_comm_world(const lh_comm* comm);
/* One grouped send + receive of device buffers, asynchronous on the context's stream (ncclGroupStart / ncclSend /
 * ncclRecv / ncclGroupEnd).  Either side may be absent (NULL / 0 bytes). */
int lh_comm_exchange(lh_comm* comm, const void* send_dev, uint64_t send_bytes, int send_peer, void* recv_dev, uint64_t recv_bytes, int recv_peer);

/* Pods as pipeline streams: the schedule that keeps every rank busy lives here, not in the host.
 * A "unit" is one Eval per stream (the prompt, or one decode step).  With Q = max(pods, world), rank r evaluates stream
 * p at unit u in tick t = u*Q + p + r; after every tick all ranks exchange once (ring shift): rank r sends what it just
 * produced to r+1 (the last rank sends the token id to rank 0) and receives what r-1 produced in the same tick.
 * pods >= world fills the pipeline (aggregate throughput); pods = 1 is the single greedy stream walking through the
 * stages (latency curve).  lh_pipeline_schedule is the pure function (no GPU): ticks as seen by `rank`, -1 = idle. */
typedef struct lh_tick { uint32_t t; int32_t stream, unit, recv_stream, recv_unit; } lh_tick;
int lh_pipeline_schedule(uint32_t rank, uint32_t world, uint32_t pods, uint32_t units, lh_tick* out, uint32_t cap); /* returns the tick count */
/* The scheduler loop itself with caller-supplied stage / exchange actions (what lh_pipeline_run executes with
 * lh_llama_stage and lh_comm_exchange plugged in): lets a host, or a CPU test over another transport, drive it. */
typedef struct lh_pipeline_hooks {
    void* user;
    int (*stage)(void* user, uint32_t stream, uint32_t unit);
    int (*exchange)(void* user, int32_t send_stream, int32_t send_unit, int32_t recv_stream, int32_t recv_unit);
} lh_pipeline_hooks;
int lh_pipeline_run_hooks(uint32_t rank, uint32_t world, uint32_t pods, uint32_t units, const lh_pipeline_hooks* hooks);

typedef struct lh_pipeline lh_pipeline;
/* pods[i]: this rank's stage of stream i (lh_llama_create with the rank's [layer0, layer1) and the stream's own KV
 * cache), all on `ctx` (one stream orders compute and p2p).  comm may be NULL when the model is not sharded.
 * The streams are dealt into G = min(pods, world) groups (more when a group would exceed the rows one weight pass takes: 64 fp32,
 * 64 block-int8 too since round 4); a group is an lh_batch - its streams advance together in ONE pass over the rank's weights - and the schedule
 * above runs over groups instead of single streams.  pods = 4 world: every tick evaluates 4 rows.  max_rows_per_tick (grouped
 * variant; 0 = as many as fit) bounds the rows of a group: 1 puts every stream into its own tick (one weight pass per stream). */
int lh_pipeline_create(lh_ctx* ctx, lh_comm* comm, lh_llama* const* pods, uint32_t n_pods, lh_pipeline** out);
int lh_pipeline_create_grouped(lh_ctx* ctx, lh_comm* comm, lh_llama* const* pods, uint32_t n_pods, uint32_t max_rows_per_tick, lh_pipeline** out);
void lh_pipeline_destroy(lh_pipeline* pl);
uint32_t lh_pipeline_groups(const lh_pipeline* pl);
/* The pure function behind the grouping (no GPU): groups for `pods` streams on `world` ranks with at most max_rows_per_tick (0 = 64)
 * streams per group; stream p belongs to group p * groups / pods. */
uint32_t lh_pipeline_group_count(uint32_t pods, uint32_t world, uint32_t max_rows_per_tick);
/* server.Do for every stream at once, greedy: if n_prompt != NULL, unit 0 evaluates prompts[i][0..n_prompt[i]) at
 * position 0 (prompts is read on rank 0 only; n_prompt on every rank); then `steps` decode units follow, each feeding
 * the argmax of the previous unit.  State (position, next token) persists across calls, so run(prompts, n, W) followed
 * by run(NULL, NULL, K) continues the same streams.  Returns after the rank's stream has drained. */
int lh_pipeline_run(lh_pipeline* pl, const uint32_t* const* prompts, const uint32_t* n_prompt, uint32_t steps);
/* The same loop as the reference runs it (pkg/server/server.go:201-204: SampleTopPTopK after every Eval): the last rank draws every
 * stream's id with the device sampler (lh_sample_params, ring of ring_size slots seeded with the prompt ids, every stream like a solo
 * lh_llama_decode_sample with the same seed) instead of the argmax.  prompts must be given on rank 0 AND on the last rank (the
 * repeat penalty needs the ring there).  run_sample(NULL, NULL, K, sp, ring) continues sampled streams. */
int lh_pipeline_run_sample(lh_pipeline* pl, const uint32_t* const* prompts, const uint32_t* n_prompt, uint32_t steps, const lh_sample_params* sp, uint32_t ring_size);
/* ModelParams.KeepCount (llama.go:47) of every stream; call it with the same value on every rank.  Past the window the streams swap context
 * like server.Do (server.go:160-172): an unsharded pipeline inside its batches' ticks, a sharded one in the unit where a stream stands at the
 * window's end - its re-fed run ((ctx - keep) / 2 tokens, the pending one last) is evaluated as one Eval at position keep by every rank in turn,
 * its residual rows travelling in front of that tick's rows in the same exchange.  Rank 0 knows the tokens (its prompts + the ids it received). */
int lh_pipeline_set_keep(lh_pipeline* pl, uint32_t keep);
/* Where the time of a run goes on THIS rank (the N > 1 curve's diagnosis): with profiling on, every tick of the following runs is bracketed
 * by HIP events on the compute stream - in front of the stage, behind it, behind the exchange - and the totals accumulate: stage_ms = the
 * rank's own kernels, exchange_ms = from the end of its stage to the end of its send / receive (RCCL: includes waiting for the predecessor's
 * data, i.e. pipeline bubbles show up here).  Three event records per tick (~ 5 us): not for the timed headline run. */
typedef struct lh_pipeline_stats { uint32_t ticks; float stage_ms, exchange_ms; } lh_pipeline_stats;
int lh_pipeline_profile(lh_pipeline* pl, int on);                      /* on: also clears the totals */
int lh_pipeline_stats_read(lh_pipeline* pl, lh_pipeline_stats* out);
/* Pre-flight of the ring: microseconds per grouped send + receive of `bytes` to the successor / from the predecessor (every rank calls it
 * at the same time; 16 KB = one 7B residual row).  SURVEY 8e expects 10-20 us per hop over xGMI. */
int lh_pipeline_hop_probe(lh_pipeline* pl, uint32_t bytes, uint32_t iters, float* us_per_hop);
/* Token ids this rank knows for a stream since creation (rank 0: received from the last rank; last rank: produced). */
int lh_pipeline_tokens(lh_pipeline* pl, uint32_t pod, uint32_t* out, uint32_t cap);

/* Time each kernel class of one decode step with HIP events on the context's stream (eager launches,
 * same kernels as the replayed graph).  Writes up to cap entries; returns the number of classes. */
typedef struct lh_kernel_time { char name[48]; uint32_t launches; float total_ms; uint64_t bytes_per_launch; } lh_kernel_time;
int lh_llama_profile_decode(lh_llama* m, uint32_t token, uint32_t past, uint32_t repeats, lh_kernel_time* out, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
