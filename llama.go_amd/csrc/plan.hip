// csrc/plan.hip — fused LLaMA plan executor: decode step (hipGraph-replayed), small-N prefill, pipeline
// stages, device-resident greedy loop, per-kernel event profiling.  Entry points: lh_llama_* (llamahip.h).
// Follows the layer schedule of llama.Eval (pkg/llama/llama.go:246-384).
#include "plan.h"
#include "kernels_llama.h"
#include "kernels_gemm.h"
#include "kernels_q8.h"
#include "kernels_skinny.h"
#include "kernels_attn.h"
#include "kernels_sample.h"
#include "kernels_stream.h"
#include "kernels_stream_q8b.h"
#include "kernels_stream_q4b.h"
#include "kernels_stream_b9.h"
#include "kernels_gemm_b9.h"
#include "kernels_rows.h"
#include "kernels_f16.h"
#include "kernels_stream_f16.h"
#include "kernels_gemm_f16.h"
#include "kernels_q4.h"
#include "kernels_attn_seg.h"
#include "kernels_attn_share.h"
#include "kernels_spec.h"
#include "feed_schedule.h"
#include "share_schedule.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <optional>
#include <type_traits>

namespace lh {

static thread_local bool g_prepare_only = false;  // set kernel attributes without launching (before graph capture)
static thread_local const char* g_only = nullptr;   // lh_llama_profile_decode: launch only the kernels of this name (timing pass)
static inline bool skip_launch(const char* name) { return g_prepare_only || (g_only && strcmp(g_only, name) != 0); }

static constexpr int TH = 1024;
static constexpr size_t FAT_LDS = 96 * 1024;  // > 80 KiB: one fat workgroup per CU

struct ProfSink {
    struct Rec { const char* name; uint64_t bytes; hipEvent_t e0, e1; };
    std::vector<Rec> recs;
    bool on = false;
};
static thread_local ProfSink* g_prof = nullptr;

// LLAMAHIP_TRACE=1: print every launch and synchronise after it (debugging aid: the last line names a faulting kernel)
static bool trace_on() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("LLAMAHIP_TRACE"); v = (e && e[0] == '1') ? 1 : 0; }
    return v == 1;
}
struct TraceScope {
    hipStream_t st;
    const char* name;
    TraceScope(hipStream_t s, const char* n) : st(s), name(n) { if (trace_on() && !g_prepare_only) { fprintf(stderr, "[lh] launch %s\n", n); fflush(stderr); } }
    ~TraceScope() {
        if (trace_on() && !g_prepare_only) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            hipStreamIsCapturing(st, &cs);
            if (cs == hipStreamCaptureStatusNone) { hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[lh]   done %s: %s\n", name, hipGetErrorString(e)); fflush(stderr); }
        }
    }
};

struct ProfScope {
    hipStream_t st;
    ProfSink::Rec rec;
    bool on;
    TraceScope tr;
    ProfScope(hipStream_t s, const char* name, uint64_t bytes) : st(s), on(g_prof && g_prof->on && !g_prepare_only), tr(s, name) {
        if (on) {
            rec.name = name; rec.bytes = bytes;
            hipEventCreate(&rec.e0); hipEventCreate(&rec.e1);
            hipEventRecord(rec.e0, st);
        }
    }
    ~ProfScope() {
        if (on) { hipEventRecord(rec.e1, st); g_prof->recs.push_back(rec); }
    }
};

// Parks the stream for `ticks` of the 100 MHz realtime counter: lh_llama_profile_decode queues its whole event/kernel sequence
// behind it, so host launch latency (event creation, API calls) does not leak into the per-kernel event intervals.
__global__ void k_park(uint64_t ticks) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

template <typename KernT>
static int set_lds_once(lh_ctx* ctx, KernT kern, size_t lds, bool* flags) {
    if (!flags[ctx->device & 15]) {
        LH_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        flags[ctx->device & 15] = true;
    }
    return 0;
}

// "This kernel is not built for the shape - take the next one": positive, so it can never be mistaken for an LH_E* code (all negative).
// Callers fall back ONLY on ST_NA; every other non-zero value is a real failure and is returned as it is.
static constexpr int ST_NA = 1;

// Grow-only device buffer of *cap elements of elem_bytes each (at least floor of them once it exists): waits for the stream (the old buffer may be in
// use), frees, allocates.  gen, where given, counts the re-allocations: a captured graph that holds the old address has it in its key and is captured
// anew (graph_cache.h).  Where a launch can be part of a stream capture the call stands in front of its prepare-only return, so that the prepare pass
// before the capture has sized the buffer (hipMalloc is not allowed under a capture).
template <typename T, typename Cap>
static int grow(lh_ctx* ctx, T** buf, Cap* cap, uint64_t need, size_t elem_bytes = sizeof(T), uint64_t floor = 0, uint64_t* gen = nullptr) {
    if (need <= *cap) return 0;
    need = std::max(need, floor);
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) LH_HIP(ctx, hipFree(*buf));
    *buf = nullptr; *cap = 0;
    if (gen) ++*gen;
    LH_HIP(ctx, hipMalloc((void**)buf, need * elem_bytes));
    *cap = (Cap)need;
    return 0;
}
static int grow_floats(lh_ctx* ctx, float** buf, uint64_t* cap, uint64_t need) { return grow(ctx, buf, cap, need); }
// the context's split-K partial products (lh_ctx::splitk; every graph whose launches may read them has splitk_gen in its key)
static int ensure_splitk(lh_ctx* ctx, uint64_t need_floats) { return grow(ctx, &ctx->splitk, &ctx->splitk_floats, need_floats, 4, 0, &ctx->splitk_gen); }

// ---- f16 <-> f32 (kernels_f16.h) ----
static inline dim3 cvt_grid(uint64_t n) { return dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((n / 4 + 255) / 256, 1), 16384)); }
int widen_f16_launch(lh_ctx* ctx, const void* src_f16, float* dst, uint64_t n) {
    if (g_prepare_only || g_only) return 0;
    TraceScope ts_(ctx->stream, "widen_f16");
    LH_TRACE("k_widen_f16");
    LH_LAUNCH(k_widen_f16, cvt_grid(n), dim3(256), 0, ctx->stream, (const _Float16*)src_f16, dst, n);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
int narrow_f16_launch(lh_ctx* ctx, const float* src, void* dst_f16, uint64_t n, unsigned long long* changed_dev) {
    LH_LAUNCH(k_narrow_f16, cvt_grid(n), dim3(256), 0, ctx->stream, src, (_Float16*)dst_f16, n, changed_dev);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// ---- block-int4 (kernels_q4.h) ----
int expand_q4_launch(lh_ctx* ctx, const void* src_q4, void* dst_q8, uint64_t n) {
    if (g_prepare_only || g_only) return 0;
    TraceScope ts_(ctx->stream, "expand_q4");
    LH_TRACE("k_expand_q4");
    const uint64_t n8 = n / 16;   // 8-byte units of the nibble plane
    LH_LAUNCH(k_expand_q4, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((n8 + 255) / 256, 1), 16384)), dim3(256), 0, ctx->stream, (const u2*)src_q4, (u4*)dst_q8, n8);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
int quantize_q4_launch(lh_ctx* ctx, const float* src, void* q, float* scales, uint64_t nblocks) {
    LH_LAUNCH(k_quantize_q4, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((nblocks + 255) / 256, 1), 65535)), dim3(256), 0, ctx->stream, src, (unsigned char*)q, scales, nblocks);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
int q4_deinterleave_launch(lh_ctx* ctx, const void* blocks, void* q, float* scales, uint64_t nblocks) {
    LH_LAUNCH(k_q4_deinterleave, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((nblocks + 255) / 256, 1), 65535)), dim3(256), 0, ctx->stream, (const unsigned int*)blocks, (unsigned char*)q, scales, nblocks);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// an image of n elements of elem_bytes each (fp32 of f16 matrices, int8 of block-int4 ones) that lives as long as the context and never moves
// (lh_ctx::wide); kind 0 = a layer's matrices, 1 = the output matrix (a layer image and an output image of the same size stay two allocations: a
// route reads both).  The element size is part of the key: an int8 image and an fp32 image of equal count do not alias.
static int wide_image(lh_ctx* ctx, uint64_t n, uint64_t elem_bytes, int kind, float** out) {
    const uint64_t key = (n << 4) | (elem_bytes << 1) | (uint64_t)kind;
    for (const auto& w : ctx->wide) if (w.first == key) { *out = w.second; return 0; }
    float* dev = nullptr;
    if (hipMalloc((void**)&dev, n * elem_bytes) != hipSuccess) LH_FAIL(ctx, LH_ENOMEM, "plan: no memory for the %s image of %s weights (%llu elements)", elem_bytes == 4 ? "fp32" : "int8", elem_bytes == 4 ? "f16" : "block-int4", (unsigned long long)n);
    ctx->wide.emplace_back(key, dev);
    *out = dev;
    return 0;
}

template <int KI, int U, int PRO, int EPI, int MAP, int THR = TH>
static int launch_gemv(lh_ctx* ctx, const GemvArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_sa<KI, U, THR, PRO, EPI, MAP>, FAT_LDS, flags);
    if (rc) return rc;
    if (skip_launch(name)) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_LAUNCH((k_gemv_sa<KI, U, THR, PRO, EPI, MAP>), dim3(ctx->ds->num_cu), dim3(THR), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

template <int KI, int U, int TPR, int PRO, int EPI, int MAP, int THR = TH>
static int launch_gemv_q8(lh_ctx* ctx, const GemvArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_q8s<KI, U, TPR, PRO, EPI, MAP, THR>, FAT_LDS, flags);   // one fat workgroup per CU (LDS request > 80 KiB)
    if (rc) return rc;
    if (skip_launch(name)) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_LAUNCH((k_gemv_q8s<KI, U, TPR, PRO, EPI, MAP, THR>), dim3(ctx->ds->num_cu), dim3(THR), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// block-int8 GEMV: pick threads-per-row so the 16-byte chunks of a row fill the lanes (K = 4096 -> 256 threads x 4 rows side by side)
template <int PRO, int EPI, int MAP>
static int gemv_q8(lh_ctx* ctx, const GemvArgs& a, const char* name) {
    if (a.K % 32 || ((EPI == EPI_QKV_ROPE || EPI == EPI_SILU_MUL) && a.M % 2))
        LH_FAIL(ctx, LH_ESHAPE, "gemv_q8 %s: K=%u must be a multiple of 32%s", name, a.K, a.M % 2 ? " and the row count even" : "");
    if ((uint64_t)a.M / ctx->ds->num_cu + 4 > (uint64_t)TH) LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv_q8 %s: M=%u exceeds %d rows per workgroup", name, a.M, TH - 4);
    const uint32_t K16 = a.K / 16;
    const uint64_t bytes = (uint64_t)a.M * a.K / 32 * 36;
    // Rows in flight per row group (x2 register sets), tools/kernel_ablate ABL_Q8S on the scalar-addressed kernel (profiles/r02_q8s_ablation.txt):
    // 22016 x 4096: U = 1 / 2 / 3 / 4 / 6 -> 21.6 / 22.2 / 21.9 / 21.3 / 21.7 us back to back, but inside the decode graph U = 4 lost to U = 2
    // (501 vs 513 tok/s same-day); 4096 x 4096: U = 1 / 2 / 4 -> 5.8 / 6.0 / 7.6 us (16 rows per CU:
    // deeper batches only add dummy loads); K = 11008: one row across the whole workgroup, U = 2 (U = 4: 13.0 vs 11.6 us)
    const uint32_t rows_wg = a.M / (uint32_t)ctx->ds->num_cu;
    // Round 3: 256-thread workgroups (ONE row group of four waves, like the fp32 stream) with U rows in flight per register set instead of
    // 1024 threads = four row groups: 489 -> 534-536 tok/s on 7B (profiles/r03_q8_workgroup_256.txt; per kernel w1|w3 24.8 -> 22.1 us, w2
    // 14.9 -> 13.4, wo 9.0 -> 8.1, lm_head 34 -> 29, wq|wk|wv 17.4 -> 16.1 with six rows).  U swept 2..8 per shape: 4 (wq|wk|wv: 6), K = 11008: 2.
    // Same threads per row, same per-lane arithmetic, same cross-wave order: results bit-identical to the 1024-thread launch.
    if (rows_wg + 4 <= 250) {
        if (K16 <= 256) return MAP == MAP_BLOCK ? launch_gemv_q8<1, 6, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes) : launch_gemv_q8<1, 4, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
        if (K16 > 512 && K16 <= 768) return launch_gemv_q8<3, 2, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
    }
    if (K16 <= 256) return rows_wg >= 32 ? launch_gemv_q8<1, 2, 256, PRO, EPI, MAP>(ctx, a, name, bytes) : launch_gemv_q8<1, 1, 256, PRO, EPI, MAP>(ctx, a, name, bytes);
    if (K16 <= 512) return launch_gemv_q8<2, 2, 256, PRO, EPI, MAP>(ctx, a, name, bytes);
    if (K16 <= 1024) return launch_gemv_q8<1, 2, 1024, PRO, EPI, MAP>(ctx, a, name, bytes);
    if (K16 <= 2048) return launch_gemv_q8<2, 2, 1024, PRO, EPI, MAP>(ctx, a, name, bytes);
    LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv_q8 %s: K=%u exceeds the supported 32768 columns", name, a.K);
}

template <int PRO, int EPI, int MAP>
static int gemv_f32(lh_ctx* ctx, const GemvArgs& a, const char* name);

template <int PRO, int EPI, int MAP>
static int gemv_f16(lh_ctx* ctx, const GemvArgs& a, const char* name);

template <int KI, int U, int TPR, int PRO, int EPI, int MAP, int THR = TH>
static int launch_gemv_q4(lh_ctx* ctx, const GemvArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_q4s<KI, U, TPR, PRO, EPI, MAP, THR>, FAT_LDS, flags);
    if (rc) return rc;
    if (skip_launch(name)) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_TRACE("k_gemv_q4s<%d,%d,%d,%d>", KI, U, TPR, THR);
    LH_LAUNCH((k_gemv_q4s<KI, U, TPR, PRO, EPI, MAP, THR>), dim3(ctx->ds->num_cu), dim3(THR), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// LLAMAHIP_Q4_U = 2 / 4 / 8: rows in flight of the K = 4096 launches (a measurement switch: the sweep of tools/bench_q4.py; README, debug switches);
// anything else: the shipped choice
static int q4_u_override() {
    static const int v = getenv("LLAMAHIP_Q4_U") ? atoi(getenv("LLAMAHIP_Q4_U")) : 0;
    return v;
}
// block-int4 GEMV (kernels_q4.h): gemv_q8's launch forms - KI, TPR and the workgroup size per shape fix the lane -> column map and the cross-wave order,
// hence the bits.  U is not part of the sums.  Only the K <= 4096 forms of 256 threads were swept; every other form (KI = 3, the 1024-thread forms,
// k_gemv_q4_rows) carries twice int8's count (a row of nibbles is half the bytes) as an UNMEASURED starting point.
template <int PRO, int EPI, int MAP>
static int gemv_q4(lh_ctx* ctx, const GemvArgs& a, const char* name) {
    if (a.K % 32 || ((EPI == EPI_QKV_ROPE || EPI == EPI_SILU_MUL) && a.M % 2))
        LH_FAIL(ctx, LH_ESHAPE, "gemv_q4 %s: K=%u must be a multiple of 32%s", name, a.K, a.M % 2 ? " and the row count even" : "");
    if ((uint64_t)a.M / ctx->ds->num_cu + 4 > (uint64_t)TH) LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv_q4 %s: M=%u exceeds %d rows per workgroup", name, a.M, TH - 4);
    const uint32_t K16 = a.K / 16;
    const uint64_t bytes = (uint64_t)a.M * a.K / 32 * 20;
    const uint32_t rows_wg = a.M / (uint32_t)ctx->ds->num_cu;
    if (rows_wg + 4 <= 250) {
        if (K16 <= 256) {
            if (q4_u_override() == 4) return launch_gemv_q4<1, 4, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            if (q4_u_override() == 2) return launch_gemv_q4<1, 2, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            if (q4_u_override() == 8) return launch_gemv_q4<1, 8, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            // (swept, tools/bench_q4.py -> profiles/q4_decode.txt: U = 4 gives the fastest decode loop of U = 2 / 4 / 8; between 4 and 8 the single launches
            // differ by less than two runs of the sweep do.  Doubling int8's counts (6 for wq|wk|wv, 4 elsewhere) bought nothing: the unpack, not the
            // bytes in flight, is what the wave waits for)
            return launch_gemv_q4<1, 4, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
        }
        if (K16 > 512 && K16 <= 768) return launch_gemv_q4<3, 4, 256, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
    }
    if (K16 <= 256) return rows_wg >= 32 ? launch_gemv_q4<1, 4, 256, PRO, EPI, MAP>(ctx, a, name, bytes) : launch_gemv_q4<1, 2, 256, PRO, EPI, MAP>(ctx, a, name, bytes);
    if (K16 <= 512) return launch_gemv_q4<2, 4, 256, PRO, EPI, MAP>(ctx, a, name, bytes);
    if (K16 <= 1024) return launch_gemv_q4<1, 4, 1024, PRO, EPI, MAP>(ctx, a, name, bytes);
    if (K16 <= 2048) return launch_gemv_q4<2, 4, 1024, PRO, EPI, MAP>(ctx, a, name, bytes);
    LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv_q4 %s: K=%u exceeds the supported 32768 columns", name, a.K);
}

template <int PRO, int EPI, int MAP>
static int gemv(lh_ctx* ctx, const GemvArgs& a, const char* name, int wtype = 0) {
    if (wtype == 1) return gemv_f16<PRO, EPI, MAP>(ctx, a, name);
    if (wtype == 2) return gemv_q4<PRO, EPI, MAP>(ctx, a, name);
    return wtype == 7 ? gemv_q8<PRO, EPI, MAP>(ctx, a, name) : gemv_f32<PRO, EPI, MAP>(ctx, a, name);
}

template <int PRO, int EPI, int MAP>
static int gemv_f32(lh_ctx* ctx, const GemvArgs& a, const char* name) {
    // rows are dealt to the workgroups in pairs (the last one takes an odd remainder); only the epilogues that combine two rows
    // (RoPE pairs, w1|w3 interleave) need an even count
    if (a.K % 4 || ((EPI == EPI_QKV_ROPE || EPI == EPI_SILU_MUL) && a.M % 2))
        LH_FAIL(ctx, LH_ESHAPE, "gemv %s: K=%u must be a multiple of 4%s", name, a.K, a.M % 2 ? " and the row count even" : "");
    const uint32_t K4 = a.K / 4;
    const uint64_t bytes = (uint64_t)a.M * a.K * 4;
    const uint32_t rows_wg = a.M / (uint32_t)ctx->ds->num_cu + 4;  // one finishing thread per row, rows * waves partial sums in LDS
    // Workgroup size and rows in flight per wave (U), same-box A/B on the decode loops (tok/s).  7B, 1024 threads:
    // U = 4 for the K = 4096 kernels 219.0, U = 2 222.8, (U at K = 4096, U at K = 11008) = (1,2) 200.0, (3,2) 220.8, (2,3) 222.4,
    // (2,1) 224.1; 512 threads (8 waves, half the per-row reductions and LDS partials), two float4 per thread at K = 4096, six at
    // K = 11008: (2,1) 226.7, (3,1) 224.5, (4,1) 223.4, (2,2) 226.1, (1,1) 209.8; 256 threads at K = 4096 (four float4 per thread): U = 2 227.7,
    // U = 3 227.0.  About 32-48 KB in flight per CU is the sweet
    // spot.  13B, 1024 threads, K = 5120: U = 4 118.8, U = 2 121.4, U = 1 120.6.
    if (K4 <= 4 * 256 && rows_wg <= 256) {  // K <= 4096: 4 waves (K = 4096: 226.0 -> 227.7 tok/s against 8 waves; no gain at K = 11008)
        switch ((K4 + 255) / 256) {
            case 1: return launch_gemv<1, 4, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            case 2: return launch_gemv<2, 4, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            case 3: return launch_gemv<3, 2, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            default: return launch_gemv<4, 2, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
        }
    }
    if (K4 <= 6 * 512 && rows_wg <= 512) {
        switch ((K4 + 511) / 512) {
            case 1: return launch_gemv<1, 2, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 2: return launch_gemv<2, 2, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 3: return launch_gemv<3, 2, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 4: return launch_gemv<4, 1, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 5: return launch_gemv<5, 1, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            default: return launch_gemv<6, 1, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
        }
    }
    if (rows_wg > (uint32_t)TH) LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv %s: M=%u exceeds %d rows per workgroup", name, a.M, TH - 4);
    switch ((K4 + TH - 1) / TH) {
        case 1: return launch_gemv<1, 2, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 2: return launch_gemv<2, 2, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 3: return launch_gemv<3, 1, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 4: return launch_gemv<4, 2, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 5: return launch_gemv<5, 2, PRO, EPI, MAP>(ctx, a, name, bytes);
        // (six float4 of x, gamma and two rows each do not fit the 128 registers of a 1024-thread workgroup next to the norm: 20 B of scratch)
        case 6: return launch_gemv<6, (PRO == PRO_RMSNORM ? 1 : 2), PRO, EPI, MAP>(ctx, a, name, bytes);
        default: LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv %s: K=%u exceeds the supported 24576 columns", name, a.K);
    }
}

// ---- f16 weight matrices (kernels_f16.h): the workgroup size and float4-per-thread count gemv_f32 picks for the shape - they fix the lane -> column
// map and the cross-wave order, hence the bits - and twice its rows in flight: a row of halves is half the bytes, and U is not part of the sums.
template <int KI, int U, int PRO, int EPI, int MAP, int THR = TH>
static int launch_gemv_h(lh_ctx* ctx, const GemvArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_sa_h<KI, U, THR, PRO, EPI, MAP>, FAT_LDS, flags);
    if (rc) return rc;
    if (skip_launch(name)) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_TRACE("k_gemv_sa_h<%d,%d,%d>", KI, U, THR);
    LH_LAUNCH((k_gemv_sa_h<KI, U, THR, PRO, EPI, MAP>), dim3(ctx->ds->num_cu), dim3(THR), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// LLAMAHIP_F16_U = 2 / 4 / 8: rows in flight of the K = 4096 launches (the sweep of tools/bench_f16.py); anything else: the shipped choice
static int f16_u_override() {
    static const int v = getenv("LLAMAHIP_F16_U") ? atoi(getenv("LLAMAHIP_F16_U")) : 0;
    return v;
}
template <int PRO, int EPI, int MAP>
static int gemv_f16(lh_ctx* ctx, const GemvArgs& a, const char* name) {
    if (a.K % 4 || ((EPI == EPI_QKV_ROPE || EPI == EPI_SILU_MUL) && a.M % 2))
        LH_FAIL(ctx, LH_ESHAPE, "gemv (f16 weights) %s: K=%u must be a multiple of 4%s", name, a.K, a.M % 2 ? " and the row count even" : "");
    const uint32_t K4 = a.K / 4;
    const uint64_t bytes = (uint64_t)a.M * a.K * 2;
    const uint32_t rows_wg = a.M / (uint32_t)ctx->ds->num_cu + 4;
    if (K4 <= 4 * 256 && rows_wg <= 256) {
        switch ((K4 + 255) / 256) {
            case 1: return launch_gemv_h<1, 8, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            case 2: return launch_gemv_h<2, 8, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            case 3: return launch_gemv_h<3, 4, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
            default:
                if (f16_u_override() == 2) return launch_gemv_h<4, 2, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
                if (f16_u_override() == 8) return launch_gemv_h<4, 8, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
                return launch_gemv_h<4, 4, PRO, EPI, MAP, 256>(ctx, a, name, bytes);
        }
    }
    if (K4 <= 6 * 512 && rows_wg <= 512) {
        switch ((K4 + 511) / 512) {
            case 1: return launch_gemv_h<1, 4, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 2: return launch_gemv_h<2, 4, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 3: return launch_gemv_h<3, 4, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 4: return launch_gemv_h<4, 2, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            case 5: return launch_gemv_h<5, 2, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
            default: return launch_gemv_h<6, 2, PRO, EPI, MAP, 512>(ctx, a, name, bytes);
        }
    }
    if (rows_wg > (uint32_t)TH) LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv (f16 weights) %s: M=%u exceeds %d rows per workgroup", name, a.M, TH - 4);
    switch ((K4 + TH - 1) / TH) {
        case 1: return launch_gemv_h<1, 4, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 2: return launch_gemv_h<2, 4, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 3: return launch_gemv_h<3, 2, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 4: return launch_gemv_h<4, 4, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 5: return launch_gemv_h<5, 4, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 6: return launch_gemv_h<6, 2, PRO, EPI, MAP>(ctx, a, name, bytes);   // (halved weight slots: two rows fit next to the norm where fp32 has one)
        default: LH_FAIL(ctx, LH_EUNSUPPORTED, "gemv (f16 weights) %s: K=%u exceeds the supported 24576 columns", name, a.K);
    }
}

// ---- 2..4 activation rows on the decode weight stream (kernels_rows.h): the same workgroup size and float4-per-thread count as the
// single-row launch of the shape (gemv_f32), so every row's sums are bit-identical to its solo decode step
template <int KI, int U, int THR, int NC, int PRO, int EPI, int MAP>
static int launch_gemv_rows(lh_ctx* ctx, const GemvRowsArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_rows<KI, U, THR, NC, PRO, EPI, MAP>, FAT_LDS, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvRowsArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_LAUNCH((k_gemv_rows<KI, U, THR, NC, PRO, EPI, MAP>), dim3(ctx->ds->num_cu), dim3(THR), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// nc = activation rows of the instantiation (2, 4, 8), norm = the launch folds the RMSNorm prologue.  Eight rows keep 8 KI float4 of
// activations per thread: they fit the 512 registers of a 256-thread workgroup's waves (K <= 4096) and, without the norm's gamma registers,
// the 256 of a 512-thread one; the other combinations would spill (ISA-checked: tools/isa_check.py) and are not built.
static bool gemv_rows_shape_ok(lh_ctx* ctx, uint32_t M, uint32_t K, uint32_t nc = 4, bool norm = false) {
    const uint32_t K4 = K / 4, rows_wg = M / (uint32_t)ctx->ds->num_cu + 4;
    if (K % 4 || M % 2) return false;
    if (K4 <= 4 * 256 && rows_wg <= 256) return true;
    if (nc > 4 && (norm || K4 > 6 * 512)) return false;
    return K4 <= 6 * 512 && rows_wg <= 512;
}
template <int NC, int PRO, int EPI, int MAP>
static int gemv_rows_nc(lh_ctx* ctx, const GemvRowsArgs& a, const char* name) {
    if (!gemv_rows_shape_ok(ctx, a.M, a.K, NC, PRO == PRO_RMSNORM)) LH_FAIL(ctx, LH_ESHAPE, "gemv_rows %s: %u x %u has no %d-row instantiation", name, a.M, a.K, NC);
    const uint32_t K4 = a.K / 4, rows_wg = a.M / (uint32_t)ctx->ds->num_cu + 4;
    const uint64_t bytes = (uint64_t)a.M * a.K * 4;
    if (K4 <= 4 * 256 && rows_wg <= 256) {
        // (eight activation rows: three / four weight rows in flight per wave measured slower than two - 5.17 / 5.40 against 4.99 ms per 8-pod tick,
        // profiles/r04_rows_kernel_u.txt)
        switch ((K4 + 255) / 256) {
            case 1: return launch_gemv_rows<1, 4, 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
            case 2: return launch_gemv_rows<2, 4, 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
            case 3: return launch_gemv_rows<3, 2, 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
            default: return launch_gemv_rows<4, 2, 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        }
    }
    if constexpr (NC > 4 && PRO == PRO_RMSNORM) return LH_ESHAPE;   // (refused above)
    else {
    switch ((K4 + 511) / 512) {
        case 1: return launch_gemv_rows<1, 2, 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 2: return launch_gemv_rows<2, 2, 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 3: return launch_gemv_rows<3, 2, 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 4: return launch_gemv_rows<4, 1, 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 5: return launch_gemv_rows<5, 1, 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        default: return launch_gemv_rows<6, 1, 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
    }
    }
}
// block-int8 twin (k_gemv_q8_rows): the launch shape of gemv_q8's 256-thread workgroups (one or three 16-quant chunks per thread).  (512 threads =
// two row groups per workgroup, two waves per SIMD: measured, nothing - 4 pods 1417 / 1333 against 1393 / 1439 tok/s, 2 pods 939 against 893;
// the kernel issues instructions 73 % of its wave cycles, it does not wait: profiles/r04_q8_rows_threads_pmc.txt)
template <int KI, int U, int NC, int PRO, int EPI, int MAP>
static int launch_gemv_q8_rows(lh_ctx* ctx, const GemvRowsArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_q8_rows<KI, U, 256, 256, NC, PRO, EPI, MAP>, FAT_LDS, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvRowsArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_LAUNCH((k_gemv_q8_rows<KI, U, 256, 256, NC, PRO, EPI, MAP>), dim3(ctx->ds->num_cu), dim3(256), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
static bool gemv_q8_rows_shape_ok(lh_ctx* ctx, uint32_t M, uint32_t K) {
    const uint32_t K16 = K / 16;
    return K % 32 == 0 && M % 2 == 0 && (K16 <= 256 || (K16 > 512 && K16 <= 768)) && (uint64_t)M / ctx->ds->num_cu + 4 <= 250;
}
template <int NC, int PRO, int EPI, int MAP>
static int gemv_q8_rows_nc(lh_ctx* ctx, const GemvRowsArgs& a, const char* name) {
    if (!gemv_q8_rows_shape_ok(ctx, a.M, a.K)) LH_FAIL(ctx, LH_ESHAPE, "gemv_q8_rows %s: %u x %u has no instantiation", name, a.M, a.K);
    const uint64_t bytes = (uint64_t)a.M * a.K / 32 * 36;
    constexpr int U = NC <= 2 ? 4 : 2;   // rows in flight per register set: the activation rows take the registers the deeper ring would
    if (a.K / 16 <= 256) return launch_gemv_q8_rows<1, U, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
    return launch_gemv_q8_rows<3, (NC <= 2 ? 2 : 1), NC, PRO, EPI, MAP>(ctx, a, name, bytes);
}
// block-int4 twin (k_gemv_q4_rows): gemv_q8_rows_nc's shapes, limits and launch forms, twice its weight rows in flight
template <int KI, int U, int NC, int PRO, int EPI, int MAP>
static int launch_gemv_q4_rows(lh_ctx* ctx, const GemvRowsArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_q4_rows<KI, U, 256, 256, NC, PRO, EPI, MAP>, FAT_LDS, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvRowsArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_TRACE("k_gemv_q4_rows<%d,%d,%d>", KI, U, NC);
    LH_LAUNCH((k_gemv_q4_rows<KI, U, 256, 256, NC, PRO, EPI, MAP>), dim3(ctx->ds->num_cu), dim3(256), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
template <int NC, int PRO, int EPI, int MAP>
static int gemv_q4_rows_nc(lh_ctx* ctx, const GemvRowsArgs& a, const char* name) {
    if (!gemv_q8_rows_shape_ok(ctx, a.M, a.K)) LH_FAIL(ctx, LH_ESHAPE, "gemv_q4_rows %s: %u x %u has no instantiation", name, a.M, a.K);
    const uint64_t bytes = (uint64_t)a.M * a.K / 32 * 20;
    constexpr int U = NC <= 2 ? 8 : 4;
    if (a.K / 16 <= 256) return launch_gemv_q4_rows<1, U, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
    return launch_gemv_q4_rows<3, (NC <= 2 ? 4 : 2), NC, PRO, EPI, MAP>(ctx, a, name, bytes);
}
// f16 twin (k_gemv_rows_h): gemv_rows_nc's shapes and limits (the activation registers are the same), twice its weight rows in flight
template <int KI, int U, int THR, int NC, int PRO, int EPI, int MAP>
static int launch_gemv_rows_h(lh_ctx* ctx, const GemvRowsArgs& a, const char* name, uint64_t bytes) {
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_gemv_rows_h<KI, U, THR, NC, PRO, EPI, MAP>, FAT_LDS, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    ProfScope ps(ctx->stream, name, bytes);
    GemvRowsArgs b = a;
    b.wg_q = (a.M / 2) / (uint32_t)ctx->ds->num_cu; b.wg_r = (a.M / 2) % (uint32_t)ctx->ds->num_cu;   // wg_row_block
    LH_TRACE("k_gemv_rows_h<%d,%d,%d,%d>", KI, U, THR, NC);
    LH_LAUNCH((k_gemv_rows_h<KI, U, THR, NC, PRO, EPI, MAP>), dim3(ctx->ds->num_cu), dim3(THR), FAT_LDS, ctx->stream, b);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
template <int NC, int PRO, int EPI, int MAP>
static int gemv_rows_h_nc(lh_ctx* ctx, const GemvRowsArgs& a, const char* name) {
    if (!gemv_rows_shape_ok(ctx, a.M, a.K, NC, PRO == PRO_RMSNORM)) LH_FAIL(ctx, LH_ESHAPE, "gemv_rows (f16 weights) %s: %u x %u has no %d-row instantiation", name, a.M, a.K, NC);
    const uint32_t K4 = a.K / 4, rows_wg = a.M / (uint32_t)ctx->ds->num_cu + 4;
    const uint64_t bytes = (uint64_t)a.M * a.K * 2;
    // (eight activation rows keep k_gemv_rows' own count: more weight rows in flight measured slower there - profiles/r04_rows_kernel_u.txt - and their
    // row bases no longer fit the scalar registers)
    if (K4 <= 4 * 256 && rows_wg <= 256) {
        switch ((K4 + 255) / 256) {
            case 1: return launch_gemv_rows_h<1, (NC > 4 ? 4 : 8), 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
            case 2: return launch_gemv_rows_h<2, (NC > 4 ? 4 : 8), 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
            case 3: return launch_gemv_rows_h<3, (NC > 4 ? 2 : 4), 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
            default: return launch_gemv_rows_h<4, (NC > 4 ? 2 : 4), 256, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        }
    }
    if constexpr (NC > 4 && PRO == PRO_RMSNORM) return LH_ESHAPE;   // (refused above)
    else {
    switch ((K4 + 511) / 512) {
        case 1: return launch_gemv_rows_h<1, (NC > 4 ? 2 : 4), 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 2: return launch_gemv_rows_h<2, (NC > 4 ? 2 : 4), 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 3: return launch_gemv_rows_h<3, (NC > 4 ? 2 : 4), 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 4: return launch_gemv_rows_h<4, (NC > 4 ? 1 : 2), 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        case 5: return launch_gemv_rows_h<5, (NC > 4 ? 1 : 2), 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
        default: return launch_gemv_rows_h<6, (NC > 4 ? 1 : 2), 512, NC, PRO, EPI, MAP>(ctx, a, name, bytes);
    }
    }
}
template <int PRO, int EPI, int MAP>
static int gemv_rows(lh_ctx* ctx, const GemvRowsArgs& a, const char* name, int wtype = 0) {
    if (wtype == 1) {
        if (a.n > 4) return gemv_rows_h_nc<8, PRO, EPI, MAP>(ctx, a, name);
        return a.n <= 2 ? gemv_rows_h_nc<2, PRO, EPI, MAP>(ctx, a, name) : gemv_rows_h_nc<4, PRO, EPI, MAP>(ctx, a, name);
    }
    if (wtype == 7) return a.n <= 2 ? gemv_q8_rows_nc<2, PRO, EPI, MAP>(ctx, a, name) : gemv_q8_rows_nc<4, PRO, EPI, MAP>(ctx, a, name);
    if (wtype == 2) return a.n <= 2 ? gemv_q4_rows_nc<2, PRO, EPI, MAP>(ctx, a, name) : gemv_q4_rows_nc<4, PRO, EPI, MAP>(ctx, a, name);
    if (a.n > 4) return gemv_rows_nc<8, PRO, EPI, MAP>(ctx, a, name);
    return a.n <= 2 ? gemv_rows_nc<2, PRO, EPI, MAP>(ctx, a, name) : gemv_rows_nc<4, PRO, EPI, MAP>(ctx, a, name);
}
// rows the decode stream carries: fp32 and f16 up to 8 (round 4; 32 FMAs per 16-byte load = a sixth of a CU's vector rate at the stream's pace),
// block-int8 and block-int4 up to 4 (their 16 converts + 16 NC FMAs per load saturate the vector ALU from there on)
static constexpr uint32_t GEMV_ROWS_MAX_F32 = 8, GEMV_ROWS_MAX_Q8 = 4;
static uint32_t gemv_rows_max(int wtype) { return wtype == 7 || wtype == 2 ? GEMV_ROWS_MAX_Q8 : GEMV_ROWS_MAX_F32; }
// every launch of a layer (and the lm_head on the last stage) has an n-row instantiation
static bool rows_path_ok(lh_ctx* ctx, const ModelDesc& m, uint32_t n) {
    if (n > gemv_rows_max(m.wtype)) return false;
    const uint32_t nc = n <= 2 ? 2 : (n <= 4 ? 4 : 8);
    // (f16: the fp32 predicate - k_gemv_rows_h keeps k_gemv_rows' activation registers and takes no more for its weight slots)
    // (block-int4: the int8 predicate - k_gemv_q4_rows takes k_gemv_q8_rows' launch forms)
    auto ok = [&](uint32_t M, uint32_t K, bool norm) { return m.wtype == 7 || m.wtype == 2 ? gemv_q8_rows_shape_ok(ctx, M, K) : ((m.wtype == 0 || m.wtype == 1) && gemv_rows_shape_ok(ctx, M, K, nc, norm)); };
    return m.hd % 2 == 0 && m.d % 4 == 0 && ok(3 * m.d, m.d, true) && ok(m.d, m.d, false) && ok(2 * m.F, m.d, true) && ok(m.d, m.F, false) && (!m.last_stage() || ok(m.V, m.d, true));
}

template <int KI, int U, int NC>
static int launch_cols(lh_ctx* ctx, const GemmColsArgs& a, const char* name) {
    auto kern = k_gemv_cols<KI, U, TH, NC>;
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, kern, FAT_LDS, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    ProfScope ps(ctx->stream, name, (uint64_t)a.M * a.K * 4);
    LH_TRACE("k_gemv_cols<%d,%d,%d,%d>", KI, U, TH, NC);
    LH_LAUNCH_AS("k_gemv_cols", kern, dim3(ctx->ds->num_cu), dim3(TH), FAT_LDS, ctx->stream, a);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// LDS-DMA kernel when every tile row starts on a 16-byte boundary (the DMA moves 16-byte granules), register-staged one otherwise
static bool gemm_dma_ok(const GemmArgs& a) {
    auto al = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    const uint32_t ldw = a.ldw ? a.ldw : a.K;
    if (a.K % GBK || a.ldx % 4 || ldw % 4 || a.xbs % 4 || a.wbs % 4 || !al(a.x)) return false;
    for (uint32_t g = 0; g < a.groups; ++g)
        if (!al(a.w[g])) return false;
    return true;
}

// Split-K for launches whose tiles do not fill the CUs evenly (prompts of <= 128 tokens are ONE row of tiles): S ranges of the contraction
// per tile, partial products summed by a second pass.  Cost model in microseconds: rounds of the busiest CU x (slabs per item + ~8 of
// prologue / epilogue) x the time of one 32-deep slab of a bn x bm tile at the CU's fp32 matrix peak (157.3 TFLOP/s / 256), plus the
// reduce pass ((S + 1) x output floats through HBM at ~4 TB/s + a launch).  S must divide the slab count and leave >= 16 slabs per item;
// a split has to win 5 %.  Not only for tiles < #CU: 344 tiles of w1|w3 at 128 rows are two rounds at 67 % occupancy, 688 half-tiles three
// rounds at 90 %.
static uint32_t pick_splitk(uint32_t tiles, uint32_t ncu, uint32_t nkf, uint32_t bn, uint32_t bm, uint64_t out_floats, double* cost_us) {
    const double slab_us = 2.0 * bn * bm * GBK / (157.3e6 / 256.0);
    double best = (double)((tiles + ncu - 1) / ncu) * (nkf + 8) * slab_us;
    uint32_t splits = 1;
    for (uint32_t s2 = 2; s2 <= 32; s2 *= 2) {
        if (nkf % s2 || nkf / s2 < 16) break;
        const double c = (double)(((uint64_t)tiles * s2 + ncu - 1) / ncu) * (nkf / s2 + 8) * slab_us + (double)(s2 + 1) * out_floats * 4.0 / 4e6 + 5.0;
        if (c < best * 0.95) { best = c; splits = s2; }
    }
    if (cost_us) *cost_us = best;
    return splits;
}

template <int WN, int WM, int TN, int TM>
static int launch_gemm(lh_ctx* ctx, const GemmArgs& a0, const char* name, uint32_t batch = 1) {
    constexpr int BN = WN * TN * 32, BM = WM * TM * 32;
    GemmArgs a = a0;
    // the DMA ring needs a few slabs to pay for its prologue and its GST-1 redundant tail slabs: short contractions (Q.K^T, K = 128)
    // stay on the register-staged kernel
    const bool dma = gemm_dma_ok(a) && a.K >= 16 * GBK;
    const uint32_t tiles = ((a.N + BN - 1) / BN) * ((a.M + BM - 1) / BM) * a.groups;
    static bool flags[2][16] = {};
    ProfScope ps(ctx->stream, name, (uint64_t)a.M * a.K * 4 * a.groups);
    if (dma) {
        // persistent: one workgroup per CU (the LDS request is padded past half a CU's 160 KB so that two never co-reside), each
        // looping over its share of the tiles x batch entries
        auto kern = k_gemm_glds<WN, WM, TN, TM>;
        const size_t lds = std::max<size_t>((size_t)GST * (BN + BM) * 32 * sizeof(float), 82 * 1024);
        int rc = set_lds_once(ctx, kern, lds, flags[1]);
        if (rc) return rc;
        if (g_prepare_only) return 0;
        a.batch = batch;
        const uint32_t ncu = (uint32_t)ctx->ds->num_cu;
        uint32_t splits = 1;
        if (!a.causal && batch == 1 && a.epi == GEMM_EPI_STORE && a.M % 4 == 0 && a.ldy % 4 == 0)
            splits = pick_splitk(tiles, ncu, a.K / GBK, BN, BM, (uint64_t)a.groups * a.N * a.M, nullptr);
        if (splits > 1) {
            if ((rc = ensure_splitk(ctx, (uint64_t)a.groups * splits * a.N * a.M))) return rc;
            a.splits = splits;
            a.part = ctx->splitk;
        }
        const uint64_t work = (uint64_t)tiles * batch * splits;
        LH_TRACE("k_gemm_glds<%d,%d,%d,%d>/s%u", WN, WM, TN, TM, splits);
        LH_LAUNCH_AS("k_gemm_glds", kern, dim3((uint32_t)std::min<uint64_t>(work, (uint64_t)ncu)), dim3(256), lds, ctx->stream, a);
        if (splits > 1) {
            const uint64_t quads = (uint64_t)a.groups * a.N * (a.M / 4);
            LH_TRACE("k_splitk_reduce");
            LH_LAUNCH(k_splitk_reduce, dim3((uint32_t)std::min<uint64_t>((quads + 255) / 256, 4096)), dim3(256), 0, ctx->stream, a);
        }
    } else {
        auto kern = k_gemm_mfma<WN, WM, TN, TM>;
        const size_t lds = (size_t)2 * GBK * (BN + 1 + BM + 1) * sizeof(float);
        int rc = set_lds_once(ctx, kern, lds, flags[0]);
        if (rc) return rc;
        if (g_prepare_only) return 0;
        LH_TRACE("k_gemm_mfma<%d,%d,%d,%d>", WN, WM, TN, TM);
        LH_LAUNCH_AS("k_gemm_mfma", kern, dim3(tiles, batch), dim3(256), lds, ctx->stream, a);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// block-int8 weights, prompts beyond 128 rows: k_gemm_q8b3 (kernels_gemm_b9.h) - X split into three bf16 planes by one pass in front, three
// exact-product MFMAs per quant block, 128 x 256 tiles.  Standalone at 1024 rows (profiles/r05_gemm_q8b3_probe.txt): 13B wq|wk|wv 524 us against
// k_gemm_q8's 1546, wo 192 / 728, w1|w3 920 / 2566, w2 477 / 1870; 7B 386 / 860, 139 / 280, 569 / 1637, 350 / 732.  One slab of its tile costs
// 0.53 of a 128 x 128 slab of k_gemm_q8 (1.2 us against 2.27): taken where rounds x that beats k_gemm_q8's own best (split-K included).
static uint16_t* ensure_xs3(lh_ctx* ctx, uint64_t elems) {
    if (elems > ctx->xs3_elems) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;
        if (ctx->xs3) hipFree(ctx->xs3);
        ctx->xs3 = nullptr; ctx->xs3_elems = 0; ctx->splitk_gen++;   // (captured graphs that hold the old planes' address are stale: same generation counter as the split-K buffer)
        if (hipMalloc((void**)&ctx->xs3, elems * 2) != hipSuccess) return nullptr;
        ctx->xs3_elems = elems;
    }
    return ctx->xs3;
}
static bool gemm_q8b3_ok(const GemmArgs& a) {
    auto al = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    if (a.N <= 64 || a.K % 128 || a.K < 16 * GBK || a.ldx % 4 || !al(a.x)) return false;
    for (uint32_t g = 0; g < a.groups; ++g)
        if (!al(a.w[g]) || !al(a.ws[g])) return false;
    return true;
}
// cost of the launch in units of (slab of a 128 x 128 k_gemm_q8 tile) x 128, and the split-K factor that gives it: a K range is a whole number
// of scale groups (4 slabs), >= 16 slabs, the ranges of a tile differ by at most one group; the reduce pass as in pick_splitk ((S + 1) x output through HBM + a launch)
static double gemm_q8b3_cost(const GemmArgs& a, uint32_t ncu, uint32_t* splits_out) {
    const uint32_t nkf = a.K / GBK, ngr = nkf / 4;
    const uint64_t tiles3 = (uint64_t)((a.N + 127) / 128) * ((a.M + 255) / 256) * a.groups;
    const double unit = 128 * 0.53, us_per_unit = 2.27 / 128.0;
    double best = (double)((tiles3 + ncu - 1) / ncu) * (nkf + 8) * unit;
    uint32_t sp = 1;
    if (a.M % 4 == 0 && a.ldy % 4 == 0)
        for (uint32_t s2 = 2; s2 <= 16; ++s2) {
            if (ngr / s2 < 4) break;                                  // a range keeps >= 16 slabs
            const uint32_t longest = 4 * ((ngr + s2 - 1) / s2);
            const double c = (double)((tiles3 * s2 + ncu - 1) / ncu) * (longest + 8) * unit + ((double)(s2 + 1) * a.groups * a.N * a.M * 4.0 / 4e6 + 5.0) / us_per_unit;
            if (c < best * 0.95) { best = c; sp = s2; }
        }
    *splits_out = sp;
    return best;
}
static int launch_gemm_q8b3(lh_ctx* ctx, GemmArgs a, const char* name, uint32_t splits) {
    auto kern = k_gemm_q8b3<4>;
    const size_t lds = gemm_q8b3_lds_bytes(4);
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, kern, lds, flags);
    if (rc) return rc;
    // (allocations BEFORE the prepare-only return, as the stream kernels do: a capture pass must find xs3 and the split-K buffer sized - ADVICE r5)
    uint16_t* xs = ensure_xs3(ctx, (uint64_t)3 * a.N * a.K);
    if (!xs) LH_FAIL(ctx, LH_ENOMEM, "%s: planes of %u x %u activations", name, a.N, a.K);
    a.xs = xs; a.xs_plane = (uint64_t)a.N * a.K; a.ldxs = a.K;
    a.splits = splits > 1 ? splits : 0; a.part = nullptr;
    if (splits > 1) {
        if ((rc = ensure_splitk(ctx, (uint64_t)a.groups * splits * a.N * a.M))) return rc;
        a.part = ctx->splitk;
    }
    if (g_prepare_only) return 0;
    {
        TraceScope ts_(ctx->stream, "split3_rows");
        Split3Args sa = {a.x, xs, a.xs_plane, a.K, a.ldx, a.K};
        LH_TRACE("k_split3_rows");
        LH_LAUNCH(k_split3_rows, dim3(a.N), dim3(256), 0, ctx->stream, sa);
    }
    const uint64_t items = (uint64_t)((a.N + 127) / 128) * ((a.M + 255) / 256) * a.groups * (splits > 1 ? splits : 1);
    ProfScope ps(ctx->stream, name, (uint64_t)a.M * a.K / 32 * 36 * a.groups);
    LH_TRACE("k_gemm_q8b3<4>/s%u", splits > 1 ? splits : 1u);
    LH_LAUNCH_AS("k_gemm_q8b3", kern, dim3((uint32_t)std::min<uint64_t>(items, (uint64_t)ctx->ds->num_cu)), dim3(512), lds, ctx->stream, a);
    if (splits > 1) {
        const uint64_t quads = (uint64_t)a.groups * a.N * (a.M / 4);
        LH_TRACE("k_splitk_reduce");
        LH_LAUNCH(k_splitk_reduce, dim3((uint32_t)std::min<uint64_t>((quads + 255) / 256, 4096)), dim3(256), 0, ctx->stream, a);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// block-int8 weights, prompts beyond the 64 rows of k_stream_q8b (and shapes it is not built for): dequantising MFMA GEMM (k_gemm_q8), persistent one workgroup per CU
static int gemm_q8_group(lh_ctx* ctx, const float* x, uint32_t ldx, uint32_t groups, const float* const* wq, const float* const* wsc, float* const* y,
                         const float* const* r, uint32_t M, uint32_t K, uint32_t n, uint32_t ldy, const char* name) {
    if (K % GBK || ldx % 4 || ((uintptr_t)x & 15)) LH_FAIL(ctx, LH_ESHAPE, "gemm_q8 %s: K=%u / ldx=%u / X alignment not supported", name, K, ldx);
    GemmArgs a = {};
    a.x = x; a.groups = groups; a.N = n; a.M = M; a.K = K; a.ldx = ldx; a.ldy = ldy;
    for (uint32_t g = 0; g < groups; ++g) { a.w[g] = wq[g]; a.ws[g] = wsc[g]; a.y[g] = y[g]; a.r[g] = r ? r[g] : nullptr; }
    // tile shape by the same balance model as the fp32 GEMM (rounds of the busiest CU x tile width); 64-row tiles up to 64 rows;
    // split-K when the launch has fewer tiles than CUs (see launch_gemm)
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, tn = (n + 127) / 128;
    auto rounds = [&](uint32_t bm) { return (double)((tn * ((M + bm - 1) / bm) * groups + ncu - 1) / ncu) * bm; };
    const int shape = n <= 64 ? 2 : rounds(160) * 1.03 < rounds(128) ? 1 : 0;
    const uint32_t bm = shape == 1 ? 160 : 128;
    const uint32_t tiles = tn * ((M + bm - 1) / bm) * groups;
    if (tiles < ncu && M % 4 == 0 && ldy % 4 == 0) {
        const uint32_t nkf = K / GBK;
        double best = (double)(nkf + 8);
        for (uint32_t s2 = 2; s2 <= 32; s2 *= 2) {
            if (nkf % s2 || nkf / s2 < 16) break;
            const double c = (double)(((uint64_t)tiles * s2 + ncu - 1) / ncu) * (nkf / s2 + 8);
            if (c < best * 0.95) { best = c; a.splits = s2; }
        }
        if (a.splits > 1) {
            if (const int rg = ensure_splitk(ctx, (uint64_t)groups * a.splits * n * M)) return rg;
            a.part = ctx->splitk;
        }
    }
    const uint32_t items = tiles * (a.splits ? a.splits : 1);
    if (gemm_q8b3_ok(a)) {
        const uint32_t nkf = K / GBK, sp = a.splits ? a.splits : 1;
        uint32_t sp3 = 1;
        const double c8 = (double)((items + ncu - 1) / ncu) * (nkf / sp + 8) * bm, c3 = gemm_q8b3_cost(a, ncu, &sp3);
        if (c3 < c8) return launch_gemm_q8b3(ctx, a, name, sp3);
    }
    ProfScope ps(ctx->stream, name, (uint64_t)M * K / 32 * 36 * groups);
    int rc;
    static bool flags[3][16] = {};
    if (shape == 1) {
        auto kern = k_gemm_q8<4, 1, 1, 5>;
        const size_t lds = std::max<size_t>((size_t)2 * (128 + 160) * 32 * sizeof(float), 82 * 1024);
        if ((rc = set_lds_once(ctx, kern, lds, flags[1]))) return rc;
        if (g_prepare_only) return 0;
        LH_TRACE("k_gemm_q8<4,1,1,5>/s%u", a.splits > 1 ? a.splits : 1u);
        LH_LAUNCH_AS("k_gemm_q8", kern, dim3(std::min<uint32_t>(items, ncu)), dim3(256), lds, ctx->stream, a);
    } else if (shape == 2) {
        auto kern = k_gemm_q8<2, 2, 1, 2>;
        const size_t lds = std::max<size_t>((size_t)2 * (64 + 128) * 32 * sizeof(float), 82 * 1024);
        if ((rc = set_lds_once(ctx, kern, lds, flags[2]))) return rc;
        if (g_prepare_only) return 0;
        LH_TRACE("k_gemm_q8<2,2,1,2>/s%u", a.splits > 1 ? a.splits : 1u);
        LH_LAUNCH_AS("k_gemm_q8", kern, dim3(std::min<uint32_t>(items, ncu)), dim3(256), lds, ctx->stream, a);
    } else {
        auto kern = k_gemm_q8<2, 2, 2, 2>;
        const size_t lds = std::max<size_t>((size_t)2 * (128 + 128) * 32 * sizeof(float), 82 * 1024);
        if ((rc = set_lds_once(ctx, kern, lds, flags[0]))) return rc;
        if (g_prepare_only) return 0;
        LH_TRACE("k_gemm_q8<2,2,2,2>/s%u", a.splits > 1 ? a.splits : 1u);
        LH_LAUNCH_AS("k_gemm_q8", kern, dim3(std::min<uint32_t>(items, ncu)), dim3(256), lds, ctx->stream, a);
    }
    if (a.splits > 1) {
        const uint64_t quads = (uint64_t)groups * n * (M / 4);
        LH_TRACE("k_splitk_reduce");
        LH_LAUNCH(k_splitk_reduce, dim3((uint32_t)std::min<uint64_t>((quads + 255) / 256, 4096)), dim3(256), 0, ctx->stream, a);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
static int gemm_q8(lh_ctx* ctx, const float* wq, const float* wsc, const float* x, float* y, const float* resid, uint32_t M, uint32_t K, uint32_t n, uint32_t ldx,
                   uint32_t ldy, const char* name) {
    return gemm_q8_group(ctx, x, ldx, 1, &wq, &wsc, &y, resid ? &resid : nullptr, M, K, n, ldy, name);
}

// Large-N prefill attention as batched MFMA GEMMs over heads, mirroring the reference's own structure (llama.go:300-333):
//   S_h = Q_h K_h^T (full block, like MulMat(K, Q))  ->  scale + causal mask + softmax  ->  V^T copy  ->  O_h = P_h V_h.
static int attention_gemm(Plan* p, const float* q, const float* kc, const float* vc, float* out, uint32_t n, uint32_t past, float scale) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    const uint32_t T = past + n, Tp = (T + 31) & ~31u, H = m.H, hd = m.hd, d = m.d;
    const uint64_t need_s = (uint64_t)H * n * Tp, need_v = (uint64_t)H * hd * Tp;
    int rc;
    if ((rc = grow_floats(ctx, &p->scores, &p->scores_cap, need_s + 32))) return rc;   // (+ the non-finite-V flag behind the scores)
    if ((rc = grow_floats(ctx, &p->vt, &p->vt_cap, need_v))) return rc;
    uint32_t* v_nonfinite = (uint32_t*)(p->scores + need_s);
    LH_TRACE("attention_gemm/hd%u/n%u", hd, n);   // (its four launches follow: the QK GEMM, k_softmax_causal, k_transpose_v, the PV GEMM; then k_attn_gemm_repair)
    {   // S[h][j][t] = sum_c Q[j][h*hd + c] * K[t][h*hd + c]
        GemmArgs a = {};
        a.x = q; a.w[0] = kc; a.y[0] = p->scores; a.groups = 1; a.N = n; a.M = T; a.K = hd; a.ldx = d; a.ldw = d; a.ldy = Tp;
        a.xbs = hd; a.wbs = hd; a.ybs = (uint64_t)n * Tp;
        a.causal = 1; a.past = past;
        if ((rc = launch_gemm<2, 2, 2, 2>(ctx, a, "attn_qk_gemm", H))) return rc;
    }
    LH_TRACE("k_softmax_causal");
    LH_LAUNCH(k_softmax_causal, dim3(n, H), dim3(256), 0, ctx->stream, p->scores, n, Tp, past, scale, v_nonfinite);
    LH_TRACE("k_transpose_v");
    LH_LAUNCH(k_transpose_v, dim3(Tp / 32, hd / 32, H), dim3(256), 0, ctx->stream, vc, p->vt, T, Tp, d, hd, v_nonfinite);
    LH_HIP(ctx, hipGetLastError());
    {   // O[j][h*hd + c] = sum_t P[h][j][t] * VT[h][c][t]
        GemmArgs a = {};
        a.x = p->scores; a.w[0] = p->vt; a.y[0] = out; a.groups = 1; a.N = n; a.M = hd; a.K = Tp; a.ldx = Tp; a.ldw = Tp; a.ldy = d;
        a.xbs = (uint64_t)n * Tp; a.wbs = (uint64_t)hd * Tp; a.ybs = hd;
        a.causal = 2; a.past = past;
        if ((rc = launch_gemm<2, 2, 2, 1>(ctx, a, "attn_pv_gemm", H))) return rc;
    }
    // a non-finite V value (k_transpose_v passed it on as 0) goes to the queries that see its key, and to no other row of the call
    LH_LAUNCH(k_attn_gemm_repair, dim3(n, H), dim3(64), 0, ctx->stream, (const float*)p->scores, vc, out, (const uint32_t*)v_nonfinite, n, Tp, past, d, hd);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// Single-pass causal prefill attention (kernels_attn.h): one kernel per layer, no score tensor, no V^T copy (+ the combine pass of the
// blocks that were cut by key range).  hd = 128 (every LLaMA size).
static int attention_flash(Plan* p, const float* q, const float* kc, const float* vc, float* out, uint32_t n, uint32_t past, float scale) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    FlashArgs a = {};
    a.q = q; a.k_cache = kc; a.v_cache = vc; a.out = out; a.d = m.d; a.H = m.H; a.n = n; a.past = past; a.scale = scale;
    a.nqb = (n + FA_BQ - 1) / FA_BQ;
    const uint32_t slots = 2u * (uint32_t)ctx->ds->num_cu;   // 64 KiB of LDS each: two workgroups per CU
    FaWork& w = p->fa_work;   // attn_worklist.h
    if (w.n != n || w.past != past) flash_work_list(w, n, past, m.H, slots);
    a.chunk = w.chunk; a.qb_cut = w.qb_cut; a.pmax = w.pmax; a.nwork = w.nwork;
    static_assert(sizeof(a.work) == sizeof(w.work), "work list");
    memcpy(a.work, w.work, sizeof(a.work));
    const bool cut = w.chunk != 0 && w.qb_cut < a.nqb;
    if (cut) {
        if (const int rg = grow_floats(ctx, &p->fa_part, &p->fa_part_cap, (uint64_t)m.H * (a.nqb - w.qb_cut) * w.pmax * FA_BQ * FA_PSTRIDE)) return rg;
        a.part = p->fa_part;
    }
    static bool flags[16] = {};
    int rc = set_lds_once(ctx, k_attn_flash, FA_LDS_BYTES, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    const uint32_t items = (a.nwork ? a.nwork : a.nqb) * m.H, grid = std::min<uint32_t>(items, slots);
    {
        ProfScope ps(ctx->stream, "attn_flash", (uint64_t)2 * (past + n) * m.d * 4);
        LH_TRACE("k_attn_flash/%s/p%u", cut ? "cut" : "uncut", cut ? w.pmax : 1u);
        LH_LAUNCH(k_attn_flash, dim3(grid), dim3(FA_TH), FA_LDS_BYTES, ctx->stream, a);
    }
    if (cut) {
        ProfScope ps(ctx->stream, "attn_flash_combine", (uint64_t)m.H * (a.nqb - w.qb_cut) * w.pmax * FA_BQ * FA_PSTRIDE * 4);
        LH_TRACE("k_attn_flash_combine/p%u", w.pmax);
        LH_LAUNCH(k_attn_flash_combine, dim3(m.H, a.nqb - w.qb_cut), dim3(256), 0, ctx->stream, a);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// groups (<= 3) weight matrices of equal shape multiplied with the same X in ONE launch (wq|wk|wv, w1|w3): more tiles per
// launch = less tile-count quantisation.  Tile shape chosen per launch: work of the busiest CU = ceil(tiles / #CU) * tile area.
// ---- short prompts, 9..64 rows: the weight-streaming MFMA kernel (kernels_stream.h) ------------------------------------------------
// up to 48 rows = three column tiles (six row tiles + three column tiles, two images: 152 KB of LDS).  Four column tiles do not fit next
// to six row tiles with 128-column chunks (with the row tiles capped at three they measured 11.4-11.9 ms at 33..64 rows, no better than
// the tile GEMM): 49..64 rows run half-length chunks (KC = 64: 2 x (6 + 4) x 16 x 68 floats = 87 KB), fp32 weights only.
// 65..96 rows (round 3): five / six column tiles on the same half-length chunks (2 x (6 + 6) x 16 x 68 floats = 104 KB; 6 x 6 accumulator tiles =
// 144 registers of the MFMA waves).  The tile GEMM's single row of 128-row tiles cost 17.6 ms at 65 rows against 10.2 ms at 64.
static constexpr uint32_t STREAM_ROWS_BUILT = 128, STREAM_ROWS_Q8 = 64, BATCH_ROWS_MAX = 64;
static constexpr uint32_t B9S_MIN_ROWS = 49, B9S_MAX_ROWS = 64;   // fp32 on k_stream_b9 (see b9s_shape_ok).  Re-checked with the final kernel, same box (profiles/
// r06_stream_b9_model_ab.txt): 17 / 32 pods 6.36 / 6.55 ms per tick on it against 5.89 / 6.11, 33 / 40 / 48 a tie (6.82 / 6.94 / 7.15 vs 6.92 / 6.97 / 7.11),
// prompts of 65..128 tokens as two passes 14.0-15.8 ms against 9.7-14.4 in one pass of k_stream_dma: the range stays 49..64
// fp32 prompts of 129..STREAM_TWO_PASS_MAX tokens: every matrix in TWO passes of the stream kernels (ceil(n / 2) rows each) instead of the tile GEMM, whose
// launches cost what 256 rows cost.  7B, ms per Eval, same box (profiles/r06_two_pass_prompts.txt): 129 / 144 / 160 / 176 / 192 tokens 17.8 / 19.4 / 19.5 / 22.2 / 22.2
// against 23.9 / 24.0 / 24.2 / 24.2 / 24.4 on the tile GEMM; from 200 tokens the two passes lose (25.1 against 24.4; 240: 28.3 against 24.7).
static constexpr uint32_t STREAM_TWO_PASS_MAX = 192;
static int stream_nct(uint32_t n) { return (int)((n + 15) / 16); }
static int stream_kc(uint32_t n) { return n <= 48 ? 128 : 64; }
static constexpr uint32_t stream_max_rows() { return STREAM_ROWS_BUILT; }

// wdt (here and down the chain): the dtype of the matrices a.w[] points at - 0 = fp32, 1 = f16 (the model's own halves: the _h kernel of the SAME
// template arguments, kernels_stream_f16.h).  Every predicate that answers ST_NA is the fp32 chain's, the LDS sizes of fp32 images included: an f16
// model must stream exactly the matrices its widened twin streams, or the two take kernels of different summation order.
template <int MAXT, int NCT, int KC>
static int launch_stream(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 0) {
    static bool flags[16] = {};
    // k_stream_mm2 (loader waves + MFMA waves, two LDS images); shapes whose two images do not fit have no launch here (round 1's kernel in which
    // every wave loaded and multiplied took them until round 6: no LLaMA shape reached it - tests/test_gpu_zz_routes.py; tools/kernels_stream_mm_r1.h)
    if (a.ws[0]) return ST_NA;   // (block-int8: k_stream_q8b)
    constexpr int KC2 = KC <= 256 ? KC : 256;
    if (stream2_lds_bytes(MAXT, NCT, KC2) > 160 * 1024) return ST_NA;
    const uint32_t grid = a.ksplit > 1 ? (uint32_t)ctx->ds->num_cu / a.ksplit * a.ksplit : (uint32_t)ctx->ds->num_cu;
    const size_t lds = std::max<size_t>(stream2_lds_bytes(MAXT, NCT, KC2), 82 * 1024);   // one workgroup per CU
    if (wdt == 1) {
        // (from two column tiles on every launch of the chain without a folded norm is k_stream_dma's: only the one-column-tile forms are built)
        if constexpr (NCT == 1) {
            static bool flags_h[16] = {};
            auto kern = k_stream_mm2_h<MAXT, NCT, KC2>;
            if (const int rh = set_lds_once(ctx, kern, lds, flags_h)) return rh;
            if (g_prepare_only) return 0;
            ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K * 2);
            LH_TRACE("k_stream_mm2_h<%d,%d,%d>/s%u", MAXT, NCT, KC2, a.ksplit > 1 ? a.ksplit : 1u);
            LH_LAUNCH_AS("k_stream_mm2_h", kern, dim3(grid), dim3(2 * ST_TH), lds, ctx->stream, a);
            LH_HIP(ctx, hipGetLastError());
            return 0;
        } else LH_FAIL(ctx, LH_EUNSUPPORTED, "%s: k_stream_mm2_h is not built for %d column tiles", name, NCT);
    }
    int rc = set_lds_once(ctx, k_stream_mm2<MAXT, NCT, KC2>, lds, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K * 4);
    LH_TRACE("k_stream_mm2<%d,%d,%d>/s%u", MAXT, NCT, KC2, a.ksplit > 1 ? a.ksplit : 1u);
    LH_LAUNCH((k_stream_mm2<MAXT, NCT, KC2>), dim3(grid), dim3(2 * ST_TH), lds, ctx->stream, a);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// ---- k_stream_dma (kernels_stream.h): fp32 weights, two column tiles on, no folded norm.  Variant = (chunk length, images in the ring,
// operand pipelining), chosen per shape by stream_dma_default_variant (the A/B switches of round 4, LLAMAHIP_STREAM_V / LLAMAHIP_ROWS_MAX, are gone:
// profiles/r04_stream_dma_variants.txt and r04_ttft_round3_paths_same_session.json keep what they measured).
constexpr int dma_nimg_fit(int maxt, int nct, int kc, int cap) {
    int n = (int)(160 * 1024 / ((size_t)(maxt + nct) * 16 * kc * 4));
    return n < cap ? n : cap;
}
// registers of an MFMA wave: the accumulator tiles + two operand sets of one k-block each (the pipeline is k-block by k-block)
constexpr bool dma_pipe_ok(int maxt, int ncw) { return maxt * ncw * 4 + 2 * (maxt + ncw) * 4 <= 210; }
template <int MAXT, int NCT, int KC, int NIMG, bool PIPE, int CS = 1>
static int launch_stream_dma(lh_ctx* ctx, const StreamArgs& a, const char* name) {
    static_assert(NIMG >= 2, "ring");
    static bool flags[16] = {};
    auto kern = k_stream_dma<MAXT, NCT, KC, NIMG, PIPE, CS>;
    const size_t lds = std::max<size_t>(stream_dma_lds_bytes(MAXT, NCT, KC, NIMG), 82 * 1024);   // one workgroup per CU
    int rc = set_lds_once(ctx, kern, lds, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    const uint32_t grid = a.ksplit > 1 ? (uint32_t)ctx->ds->num_cu / a.ksplit * a.ksplit : (uint32_t)ctx->ds->num_cu;
    ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K * 4);
    LH_TRACE("k_stream_dma<%d,%d,%d,%d,%d,%d>/s%u", MAXT, NCT, KC, NIMG, (int)PIPE, CS, a.ksplit > 1 ? a.ksplit : 1u);
    LH_LAUNCH_AS("k_stream_dma", kern, dim3(grid), dim3(2 * ST_TH), lds, ctx->stream, a);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// k_stream_dma_h (kernels_stream_f16.h): the same shape on f16 weights.  Ring depth: the weight part of an image is half as large, so more images fit;
// shipped: as many as fit up to four with 64-column chunks (the fp32 cap) and up to three with 128-column chunks (fp32: the two that fit).  Probe builds
// (-DSTREAM_H_NIMG64=5; -DSTREAM_H_NIMG64=3 -DSTREAM_H_NIMG128=2) measured within 2 % of these at 9..160 rows, no consistent winner
// (profiles/f16_stream.txt); the sums do not depend on the depth.
#ifndef STREAM_H_NIMG64
#define STREAM_H_NIMG64 4
#endif
#ifndef STREAM_H_NIMG128
#define STREAM_H_NIMG128 3
#endif
constexpr int dma_h_nimg_fit(int maxt, int nct, int kc, int cap) {
    int n = (int)(160 * 1024 / stream_dma_h_image_bytes(maxt, nct, kc));
    return n < cap ? n : cap;
}
template <int MAXT, int NCT, int KC, int CS = 1>
static int launch_stream_dma_h(lh_ctx* ctx, const StreamArgs& a, const char* name) {
    constexpr int NIMG = dma_h_nimg_fit(MAXT, NCT, KC, KC == 64 ? STREAM_H_NIMG64 : STREAM_H_NIMG128);
    static_assert(NIMG >= 2, "ring");
    static bool flags[16] = {};
    auto kern = k_stream_dma_h<MAXT, NCT, KC, NIMG, false, CS>;
    const size_t lds = std::max<size_t>((size_t)NIMG * stream_dma_h_image_bytes(MAXT, NCT, KC), 82 * 1024);   // one workgroup per CU
    int rc = set_lds_once(ctx, kern, lds, flags);
    if (rc) return rc;
    if (g_prepare_only) return 0;
    const uint32_t grid = a.ksplit > 1 ? (uint32_t)ctx->ds->num_cu / a.ksplit * a.ksplit : (uint32_t)ctx->ds->num_cu;
    ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K * 2);
    LH_TRACE("k_stream_dma_h<%d,%d,%d,%d,%d,%d>/s%u", MAXT, NCT, KC, NIMG, 0, CS, a.ksplit > 1 ? a.ksplit : 1u);
    LH_LAUNCH_AS("k_stream_dma_h", kern, dim3(grid), dim3(2 * ST_TH), lds, ctx->stream, a);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// variants: 0 = 64-column chunks, as many images as fit (<= 4); 2 = 128-column chunks, two images; 1 / 3 = the same with pipelined operands
// (measured round 4, profiles/r04_stream_dma_variants.txt: the operand pipeline buys nothing on two to six column tiles - the LDS
// latency behind a barrier is not what idles the matrix pipe - so only the eight-column-tile launches are built with it)
template <int MAXT, int NCT>
static int launch_stream_dma_v(lh_ctx* ctx, const StreamArgs& a, const char* name, int v, int wdt = 0) {
    constexpr int N64 = dma_nimg_fit(MAXT, NCT, 64, 4), N128 = dma_nimg_fit(MAXT, NCT, 128, 2);
    static_assert(N64 >= 2, "two images of 64-column chunks always fit");
    if (wdt == 1) {   // the chunk length and the column split the fp32 branch below picks (the operand pipeline, v == 1, is no shipped default: not built)
        if (v != 0 && v != 2) LH_FAIL(ctx, LH_EUNSUPPORTED, "%s: k_stream_dma_h has no pipelined variant", name);
        if constexpr (NCT == 8) return launch_stream_dma_h<MAXT, NCT, 64, 2>(ctx, a, name);
        else if constexpr (NCT == 7) return launch_stream_dma_h<MAXT, NCT, 64>(ctx, a, name);
        else {
            if constexpr (N128 >= 2) if (v == 2) return launch_stream_dma_h<MAXT, NCT, 128>(ctx, a, name);
            return launch_stream_dma_h<MAXT, NCT, 64>(ctx, a, name);
        }
    }
    if constexpr (NCT == 8) {   // eight column tiles: MFMA waves as 2 K-groups x 2 column halves, 64-column chunks
        static_assert(dma_pipe_ok(MAXT, NCT / 2), "column split");
        if (v == 1) return launch_stream_dma<MAXT, NCT, 64, N64, true, 2>(ctx, a, name);
        return launch_stream_dma<MAXT, NCT, 64, N64, false, 2>(ctx, a, name);
    } else if constexpr (NCT == 7) {   // seven (97..112 rows): the four K-groups still hold MAXT x 7 accumulator tiles (168 + 52 operand registers at six row tiles)
        return launch_stream_dma<MAXT, NCT, 64, N64, false>(ctx, a, name);
    } else {
        if constexpr (N128 >= 2) if (v == 2) return launch_stream_dma<MAXT, NCT, 128, 2, false>(ctx, a, name);
        return launch_stream_dma<MAXT, NCT, 64, N64, false>(ctx, a, name);
    }
}
// per shape (7B launches, same box, tools/stream_mm_check mode 4): long chunks where a workgroup streams five or more row tiles next to two
// column tiles (w1|w3 at 17..32 rows: 63.2 us against 67.2-68.4; memory-bound there, and a DMA instruction then moves 512 contiguous bytes
// of a row); everywhere else the deeper ring of short chunks (wq|wk|wv at 32 rows 36.6 against 37.1, wo 19.1 against 25.6, w2 46.5 against 67.2)
static int stream_dma_default_variant(int maxt, int nct) { return (nct == 2 && maxt >= 5) ? 2 : 0; }   // (eight column tiles: the operand pipeline measured 2-5 % slower)
// K-chunk: 128 columns; 256 for single-tile workgroups on long rows (w2: 37.5 -> 34.9 us).  Longer chunks (a whole 1 KB of ONE row per
// load instruction, more bytes in flight) measured slower on the other 7B shapes, and a chunk-major copy of the weights (contiguous
// runs per workgroup) gained 2-13 % at twice the footprint: profiles/r02c_stream_mm_check.txt.
template <int MAXT, int NCT>
static int launch_stream_kc(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 0) {
    if constexpr (NCT >= 4) return launch_stream<MAXT, NCT, 64>(ctx, a, name, wdt);
    else {
        if (MAXT == 1 && a.K > 4096 && a.K % 256 == 0) return launch_stream<MAXT, NCT, (MAXT == 1 ? 256 : 128)>(ctx, a, name, wdt);
        return launch_stream<MAXT, NCT, 128>(ctx, a, name, wdt);
    }
}
template <int MAXT, int NCT>
static int launch_stream_nct(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 0) {
    // (one column tile, 9..16 rows, stays on k_stream_mm2 with the norm folded into the launch.  Round 5 built the sixteen-equal-waves LDS-DMA
    // structure of k_stream_q8b for it, norm folded on the operand-read side (tools/kernels_stream_eq.h): correct, and slower on every 7B launch -
    // w1|w3 72.0 us against 66-67, wq|wk|wv 43.3 / 39.5, wo 32.0 / 17.6, w2 79.3 / 37.6 at 16 rows - a workgroup barrier of sixteen waves costs
    // ~0.45 us and fp32 chunks that fit the ring are 64 columns: 64..172 barriers per launch.  profiles/r05_stream_eq_probe.txt)
    if constexpr (NCT >= 2) {
        // (one column tile, 9..16 rows, stays on k_stream_mm2 with the norm folded into the launch: on the LDS-DMA kernel with the norm's own launch
        // in front it measured 6.12-6.14 ms per Eval against 5.63-5.68, 16 pods 5.91 against 5.81 ms per tick - profiles/r04_stream_one_column_tile_probe.txt)
        if (!a.ws[0] && !a.gamma && !a.tiled) return launch_stream_dma_v<MAXT, NCT>(ctx, a, name, stream_dma_default_variant(MAXT, NCT), wdt);
    }
    if constexpr (NCT > 6) return ST_NA;   // (k_stream_mm2 holds MAXT x NCT accumulator tiles per wave: up to six column tiles)
    else return launch_stream_kc<MAXT, NCT>(ctx, a, name, wdt);
}
template <int MAXT>
static int launch_stream_n(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 0) {
    if (a.n <= 16) return launch_stream_nct<MAXT, 1>(ctx, a, name, wdt);
    if (a.n <= 32) return launch_stream_nct<MAXT, 2>(ctx, a, name, wdt);
    if (a.n <= 48) return launch_stream_nct<MAXT, 3>(ctx, a, name, wdt);
    if (a.n <= 64) return launch_stream_nct<MAXT, 4>(ctx, a, name, wdt);
    if constexpr (MAXT <= 6) {   // (8 x 5 / 8 x 6 accumulator tiles do not fit the registers: those launches take the tile GEMM)
        if (a.n <= 80) return launch_stream_nct<MAXT, 5>(ctx, a, name, wdt);
        if (a.n <= 96) return launch_stream_nct<MAXT, 6>(ctx, a, name, wdt);
        if (a.n <= 112) return launch_stream_nct<MAXT, 7>(ctx, a, name, wdt);   // 97..128 rows (round 4): seven / eight column tiles, fp32 weights only
        return launch_stream_nct<MAXT, 8>(ctx, a, name, wdt);
    }
    return ST_NA;
}
// Row tiles of a workgroup -> the instantiation built for them: one to four as they are, five and six on the six-tile build, seven and eight on the
// eight-tile one (0: none; the callers refuse more than eight before they come here, and a matrix has at least one tile).
static int stream_maxt_built(uint32_t maxt) { return maxt <= 4 ? (int)maxt : maxt <= 6 ? 6 : maxt <= 8 ? 8 : 0; }
// f(std::integral_constant<int, MAXT>()) for that instantiation: the one switch behind the launchers of k_stream_mm2 / _dma, k_stream_q8b and k_stream_b9
template <typename F>
static int with_stream_maxt(uint32_t maxt, F&& f) {
    switch (stream_maxt_built(maxt)) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 6: return f(std::integral_constant<int, 6>());
        case 8: return f(std::integral_constant<int, 8>());
        default: return ST_NA;
    }
}
static int launch_stream_maxt(lh_ctx* ctx, const StreamArgs& a, const char* name, uint32_t maxt, int wdt = 0) {
    return with_stream_maxt(maxt, [&](auto mt) { return launch_stream_n<decltype(mt)::value>(ctx, a, name, wdt); });
}
// returns ST_NA when the shape is not one the kernel is built for (the caller then takes the tile GEMM)
static int gemm_stream_group(lh_ctx* ctx, const float* x, uint32_t ldx, uint32_t groups, const float* const* w, float* const* y, const float* const* r, uint32_t M,
                             uint32_t K, uint32_t n, uint32_t ldy, const char* name, const StreamArgs* fused = nullptr, int wdt = 0) {
    if (n > stream_max_rows() || groups > 3 || M % 16 || K % 128 || ldx % 4 || ldy % 4 || ((uintptr_t)x & 15)) return ST_NA;
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, T = M / 16 * groups;
    // ST_EPI_SILU_MUL deals (w1, w3) tile pairs: twice the pairs' ceiling
    const uint32_t maxt = (fused && fused->epi == ST_EPI_SILU_MUL) ? 2 * ((M / 16 + ncu - 1) / ncu) : (T + ncu - 1) / ncu;
    if (maxt > 8) return ST_NA;
    if (fused && fused->epi != ST_EPI_STORE) {   // the fused epilogues live in the wave-specialised variant only: its two images must fit
        if (stream2_lds_bytes(stream_maxt_built(maxt), stream_nct(n), stream_kc(n)) > 160 * 1024) return ST_NA;
        if (fused->epi == ST_EPI_QKV_ROPE && (fused->hd % 4 || M % fused->hd)) return ST_NA;
    }
    StreamArgs a = {};
    if (fused) a = *fused;
    a.x = x; a.groups = groups; a.M = M; a.K = K; a.n = n; a.ldx = ldx; a.ldy = ldy;
    for (uint32_t g = 0; g < groups; ++g) {
        a.w[g] = w[g]; a.y[g] = y ? y[g] : nullptr; a.r[g] = r ? r[g] : nullptr;
        if (((uintptr_t)w[g] & 15) || ((uintptr_t)a.y[g] & 15) || (a.r[g] && ((uintptr_t)a.r[g] & 15))) return ST_NA;
    }
    return launch_stream_maxt(ctx, a, name, maxt, wdt);
}

// Single-tile matrices (wo, w2: one 16-row tile per CU) at 17..48 rows: pairs of workgroups split the contraction (StreamArgs::ksplit), so a
// workgroup re-reads half of X out of L2 for twice the rows, and k_stream_reduce_norm adds the two partials + the residual and
// writes the RMSNorm * gamma rows the NEXT matmul reads - it stands where that norm's launch stood.  Standalone, 32 rows (tools/
// stream_mm_check, profiles/r02d_stream_ksplit.txt): w2 55.6 -> 45.6 us, wo 23.9 -> 22.0 us; at 16 rows nothing (37.7 -> 37.0, 17.9 -> 21.1).
// returns ST_NA when not applicable (the caller takes the one-launch path).
static int gemm_stream_split(lh_ctx* ctx, const float* w, const float* x, uint32_t ldx, uint32_t M, uint32_t K, uint32_t n, const float* resid,
                             float* y, const float* gamma, float* h, const char* name, int wdt = 0) {
    // pairs: four-way splits measured no better, standalone (w2 at 32 / 48 rows: 45.6 / 62.2 us in pairs, 47.6 / 60.6 in fours, + a longer
    // reduce pass) and in the model (40 / 48 tokens: 8.94 / 9.01 ms vs 9.08 / 9.24)
    const uint32_t S = 2u;
    if (n <= 16 || n > stream_max_rows() || M % 16 || M > 8192 || K % 128 || K / 128 < 4 * S || ldx % 4) return ST_NA;
    if ((((uintptr_t)w | (uintptr_t)x | (uintptr_t)y | (uintptr_t)resid | (uintptr_t)gamma | (uintptr_t)h) & 15)) return ST_NA;
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, ngrp = ncu / S;
    if (ngrp == 0) return ST_NA;
    const uint32_t maxt = (M / 16 + ngrp - 1) / ngrp;
    if (maxt > 8) return ST_NA;
    if (stream2_lds_bytes(stream_maxt_built(maxt), stream_nct(n), stream_kc(n)) > 160 * 1024) return ST_NA;
    if (const int rg = ensure_splitk(ctx, (uint64_t)S * n * M)) return rg;
    StreamArgs a = {};
    a.x = x; a.groups = 1; a.M = M; a.K = K; a.n = n; a.ldx = ldx; a.ldy = M; a.w[0] = w; a.y[0] = ctx->splitk;
    a.ksplit = S; a.ysplit = (uint64_t)n * M;
    const int rs = launch_stream_maxt(ctx, a, name, maxt, wdt);
    if (rs) return rs;
    if (g_prepare_only) return 0;
    StreamReduceArgs r = {};
    r.part = ctx->splitk; r.stride = a.ysplit; r.resid = resid; r.y = y; r.gamma = gamma; r.h = h; r.S = S; r.d = M; r.ldy = M;
    { TraceScope ts_(ctx->stream, "stream_reduce_norm"); LH_LAUNCH(k_stream_reduce_norm, dim3(n), dim3(256), 0, ctx->stream, r); }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// ---- k_stream_q8b (kernels_stream_q8b.h, round 5): block-int8 weights on the bf16 matrix pipe, activations as three bf16 planes (exact split).
// Chunk length per shape: 256 columns; 512 where a workgroup holds at most three row tiles next to one column tile (wq|wk|wv: half as many
// barriers; standalone on 7B 20.2-22.2 us against 23.5); 128 from three column tiles on and where K is not a multiple of 256.
constexpr int q8b_nimg_fit(int maxt, int xr, int kc) {
    const int n = (int)(160 * 1024 / stream_q8b_image_bytes(maxt, xr, kc));
    return n < 3 ? n : 3;   // (a fourth image measured 1-4 % slower on every 7B launch where it fits, profiles/r05_q8b_probe.txt)
}
// wdt (here and down the chain): the dtype of the matrices a.w[] points at - 7 = the int8 quants, 2 = the nibble planes of a block-int4 model (k_stream_q4b,
// kernels_stream_q4b.h: the kernel of the SAME MAXT, NCT, KC and XR).  Every predicate that answers ST_NA and every choice that reaches the sums - MAXT,
// NCT / XR, KC with its q8b_nimg_fit conditions, the K-split - is the int8 chain's, taken from the INT8 image's sizes: a block-int4 model must take exactly
// the launches its expanded twin takes.  Only the ring depth is the 4-bit kernel's own: as many of its smaller images as fit in 160 KB, up to Q4B_NIMG_CAP.
// Shipped: three, the int8 cap, which gives a third image to the shapes whose int8 ring holds two; whether a fourth (-DQ4B_NIMG_CAP=4) is slower as it
// measured for int8 is recorded in profiles/q4_stream.txt.  The sums do not depend on the depth.
#ifndef Q4B_NIMG_CAP
#define Q4B_NIMG_CAP 3
#endif
constexpr int q4b_nimg_fit(int maxt, int xr, int kc) {
    const int n = (int)(160 * 1024 / stream_q4b_image_bytes(maxt, xr, kc));
    return n < Q4B_NIMG_CAP ? n : Q4B_NIMG_CAP;
}
template <int MAXT, int NCT, int KC, int XR>
static int launch_stream_q8b(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 7) {
    constexpr int NIMG = q8b_nimg_fit(MAXT, XR, KC);
    if constexpr (NIMG < 2) return ST_NA;
    else if (wdt == 2) {
        constexpr int NIMG4 = q4b_nimg_fit(MAXT, XR, KC);
        static_assert(NIMG4 >= NIMG, "the 4-bit image is the smaller one");
        static bool flags4[16] = {};
        auto kern = k_stream_q4b<MAXT, NCT, KC, NIMG4, XR>;
        const size_t lds = std::max<size_t>((size_t)NIMG4 * stream_q4b_image_bytes(MAXT, XR, KC), 82 * 1024);   // one workgroup per CU
        int rc = set_lds_once(ctx, kern, lds, flags4);
        if (rc) return rc;
        if (g_prepare_only) return 0;
        const uint32_t grid = a.ksplit > 1 ? (uint32_t)ctx->ds->num_cu / a.ksplit * a.ksplit : (uint32_t)ctx->ds->num_cu;
        ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K / 32 * 20);
        LH_TRACE("k_stream_q4b<%d,%d,%d,%d,%d>/s%u", MAXT, NCT, KC, NIMG4, XR, a.ksplit > 1 ? a.ksplit : 1u);
        LH_LAUNCH_AS("k_stream_q4b", kern, dim3(grid), dim3(Q8B_TH), lds, ctx->stream, a);
        LH_HIP(ctx, hipGetLastError());
        return 0;
    } else {
        static bool flags[16] = {};
        auto kern = k_stream_q8b<MAXT, NCT, KC, NIMG, XR>;
        const size_t lds = std::max<size_t>((size_t)NIMG * stream_q8b_image_bytes(MAXT, XR, KC), 82 * 1024);   // one workgroup per CU
        int rc = set_lds_once(ctx, kern, lds, flags);
        if (rc) return rc;
        if (g_prepare_only) return 0;
        const uint32_t grid = a.ksplit > 1 ? (uint32_t)ctx->ds->num_cu / a.ksplit * a.ksplit : (uint32_t)ctx->ds->num_cu;
        ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K / 32 * 36);
        LH_TRACE("k_stream_q8b<%d,%d,%d,%d,%d>/s%u", MAXT, NCT, KC, NIMG, XR, a.ksplit > 1 ? a.ksplit : 1u);
        LH_LAUNCH_AS("k_stream_q8b", kern, dim3(grid), dim3(Q8B_TH), lds, ctx->stream, a);
        LH_HIP(ctx, hipGetLastError());
        return 0;
    }
}
template <int MAXT, int NCT, int XR>
static int launch_stream_q8b_kc(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 7) {
    const uint32_t S = a.ksplit > 1 ? a.ksplit : 1u;
    if constexpr (NCT == 1 && MAXT <= 3 && q8b_nimg_fit(MAXT, XR, 512) >= 2) { if (a.K % 512 == 0 && a.K / 512 >= S) return launch_stream_q8b<MAXT, NCT, 512, XR>(ctx, a, name, wdt); }
    if constexpr (NCT <= 2 && q8b_nimg_fit(MAXT, XR, 256) >= 2) { if (a.K % 256 == 0 && a.K / 256 >= S) return launch_stream_q8b<MAXT, NCT, 256, XR>(ctx, a, name, wdt); }
    if (a.K / 128 < S) return ST_NA;
    return launch_stream_q8b<MAXT, NCT, 128, XR>(ctx, a, name, wdt);
}
template <int MAXT>
static int launch_stream_q8b_n(lh_ctx* ctx, const StreamArgs& a, const char* name, int wdt = 7) {
    if (a.n <= 8) return launch_stream_q8b_kc<MAXT, 1, 8>(ctx, a, name, wdt);
    if (a.n <= 16) return launch_stream_q8b_kc<MAXT, 1, 16>(ctx, a, name, wdt);
    if (a.n <= 32) return launch_stream_q8b_kc<MAXT, 2, 32>(ctx, a, name, wdt);
    if (a.n <= 48) return launch_stream_q8b_kc<MAXT, 3, 48>(ctx, a, name, wdt);
    if (a.n <= 64) return launch_stream_q8b_kc<MAXT, 4, 64>(ctx, a, name, wdt);
    return ST_NA;
}
static int launch_stream_q8b_maxt(lh_ctx* ctx, const StreamArgs& a, const char* name, uint32_t maxt, int wdt = 7) {
    return with_stream_maxt(maxt, [&](auto mt) { return launch_stream_q8b_n<decltype(mt)::value>(ctx, a, name, wdt); });
}
// ---- k_stream_b9 (kernels_stream_b9.h, round 6): fp32 weights x the same three bf16 planes, eight of the nine exact bf16 products per weight on the bf16 matrix pipe.
// Wave-specialised like k_stream_dma (four loader waves, four MFMA waves); up to four column tiles (64 rows), 64-column chunks, as many images
// as fit (<= 4).  Eight row tiles next to four column tiles are not built (the MFMA waves' 4 x 4 accumulator tiles + operands spill).
// Eight of the nine products: xl * wl (<= 2^-32 of its product, far below the fp32 accumulator's own rounding) is dropped - against an f64 product max and
// rms error are unchanged to four digits (tools/b9s_probe, profiles/r06_stream_b9_probe.txt: 7B w1|w3 at 64 rows 1.102e-05 / 6.295e-07 with nine and
// with eight), and the kernel is power-bound (the chip holds 1.6-1.9 GHz under it), so an MFMA saved is time saved: 92.2 -> 88.0 us.  Six products
// (also xm * wl and xl * wm, 2^-24 each) measured 79.8 us at rms 6.311e-07 - not taken: those terms are the size of an fp32 product's own rounding.
static constexpr int B9S_PRODUCTS = 8;
template <int MAXT, int NCT>
static int launch_stream_b9(lh_ctx* ctx, const StreamArgs& a, const char* name) {
    constexpr int NIMG = stream_b9_nimg(MAXT, NCT, 4);
    if constexpr (NIMG < 2 || (MAXT >= 8 && NCT >= 4)) return ST_NA;
    else {
        static bool flags[16] = {};
        auto kern = k_stream_b9<MAXT, NCT, NIMG, B9S_PRODUCTS>;
        const size_t lds = std::max<size_t>((size_t)NIMG * stream_b9_image_bytes(MAXT, NCT), 82 * 1024);   // one workgroup per CU
        int rc = set_lds_once(ctx, kern, lds, flags);
        if (rc) return rc;
        if (g_prepare_only) return 0;
        const uint32_t grid = a.ksplit > 1 ? (uint32_t)ctx->ds->num_cu / a.ksplit * a.ksplit : (uint32_t)ctx->ds->num_cu;
        ProfScope ps(ctx->stream, name, (uint64_t)a.groups * a.M * a.K * 4);
        LH_TRACE("k_stream_b9<%d,%d,%d,%d>/s%u", MAXT, NCT, NIMG, B9S_PRODUCTS, a.ksplit > 1 ? a.ksplit : 1u);
        LH_LAUNCH_AS("k_stream_b9", kern, dim3(grid), dim3(B9S_TH), lds, ctx->stream, a);
        LH_HIP(ctx, hipGetLastError());
        return 0;
    }
}
template <int MAXT>
static int launch_stream_b9_n(lh_ctx* ctx, const StreamArgs& a, const char* name) {
    if (a.K % B9S_KC || a.K / B9S_KC < (a.ksplit > 1 ? a.ksplit : 1u)) return ST_NA;
    if (a.n <= 16) return launch_stream_b9<MAXT, 1>(ctx, a, name);
    if (a.n <= 32) return launch_stream_b9<MAXT, 2>(ctx, a, name);
    if (a.n <= 48) return launch_stream_b9<MAXT, 3>(ctx, a, name);
    if (a.n <= 64) return launch_stream_b9<MAXT, 4>(ctx, a, name);
    return ST_NA;
}
static int launch_stream_b9_maxt(lh_ctx* ctx, const StreamArgs& a, const char* name, uint32_t maxt) {
    return with_stream_maxt(maxt, [&](auto mt) { return launch_stream_b9_n<decltype(mt)::value>(ctx, a, name); });
}
static bool stream_b9_built(uint32_t maxt, uint32_t n) { return maxt >= 1 && maxt <= 8 && n >= 1 && n <= 64 && !(maxt > 6 && n > 48); }
// groups (<= 3) matrices of equal shape - block-int8 (wsc: their scale planes) or fp32 (wsc[g] == nullptr: k_stream_b9) - times the same activation
// planes in ONE launch; fused: the epilogue (RoPE + cache append | silu * mul).  wdt = 2: wq[] are the nibble planes of a block-int4 model (the alignment
// checks below then hold for the nibble planes' addresses).
static int gemm_q8b_group(lh_ctx* ctx, const uint16_t* xs, uint64_t xs_plane, uint32_t ldxs, uint32_t groups, const float* const* wq, const float* const* wsc, float* const* y,
                          const float* const* r, uint32_t M, uint32_t K, uint32_t n, uint32_t ldy, const char* name, const StreamArgs* fused = nullptr, int wdt = 7) {
    if (n == 0 || n > STREAM_ROWS_Q8 || groups > 3 || M % 16 || K % 128 || ldxs % 8 || ldy % 4 || ((uintptr_t)xs & 15) || (xs_plane * 2) % 16) return ST_NA;
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, T = M / 16 * groups;
    const uint32_t maxt = (fused && fused->epi == ST_EPI_SILU_MUL) ? 2 * ((M / 16 + ncu - 1) / ncu) : (T + ncu - 1) / ncu;
    if (maxt > 8) return ST_NA;
    if (fused && fused->epi == ST_EPI_QKV_ROPE && (fused->hd % 4 || M % fused->hd)) return ST_NA;
    StreamArgs a = {};
    if (fused) a = *fused;
    a.xs = xs; a.xs_plane = xs_plane; a.ldxs = ldxs; a.groups = groups; a.M = M; a.K = K; a.n = n; a.ldy = ldy;
    for (uint32_t g = 0; g < groups; ++g) {
        a.w[g] = wq[g]; a.ws[g] = wsc[g]; a.y[g] = y ? y[g] : nullptr; a.r[g] = r ? r[g] : nullptr;
        if (((uintptr_t)wq[g] & 15) || ((uintptr_t)a.y[g] & 15) || (a.r[g] && ((uintptr_t)a.r[g] & 15)) || ((uintptr_t)a.ws[g] & 15)) return ST_NA;
    }
    return a.ws[0] ? launch_stream_q8b_maxt(ctx, a, name, maxt, wdt) : launch_stream_b9_maxt(ctx, a, name, maxt);
}
// One matrix as groups of S workgroups that split the contraction (a workgroup then holds S times the rows for a 1 / S of K: the single-tile
// matrices wo and w2 read S times less of X out of L2 and run S times fewer, longer chunk loops), k_stream_reduce_norm adds the S partials +
// the residual in fixed order and writes the RMSNorm * gamma rows of the NEXT matmul as planes (and as fp32 rows when h is given) - it
// stands where that norm's launch stood.  Standalone, 7B (profiles/r05_q8b_probe.txt): wo at 8 / 32 rows 11.5 / 14.5 us in fours against
// 12.5 / - unsplit, w2 17.5 / 26.2 against 20.3 / 39.6.
static uint32_t q8b_split_groups(uint32_t nchunks, uint32_t ncu) {   // S: fours, halved while a workgroup's share of the contraction would fall under two chunks
    uint32_t S = 4;
    while (S > 1 && (nchunks < 2 * S || ncu / S == 0)) S >>= 1;
    return S;
}
static int gemm_q8b_split(lh_ctx* ctx, const float* wq, const float* wsc, const uint16_t* xs, uint64_t xs_plane, uint32_t ldxs, uint32_t M, uint32_t K, uint32_t n,
                          const float* resid, float* y, const float* gamma, float* h, uint16_t* hs, uint64_t hs_plane, const char* name, int wdt = 7) {
    if (n == 0 || n > STREAM_ROWS_Q8 || M % 16 || M > 8192 || M % 4 || K % 128 || ldxs % 8 || ((uintptr_t)xs & 15) || (xs_plane * 2) % 16) return ST_NA;
    if ((((uintptr_t)wq | (uintptr_t)y | (uintptr_t)resid | (uintptr_t)gamma | (uintptr_t)h | (uintptr_t)hs | (uintptr_t)wsc) & 15)) return ST_NA;
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, nchunks = wsc ? K / (K % 256 == 0 ? 256u : 128u) : K / (uint32_t)B9S_KC;
    const uint32_t S = q8b_split_groups(nchunks, ncu), ngrp = ncu / S, maxt = (M / 16 + ngrp - 1) / ngrp;
    if (maxt > 8) return ST_NA;
    if (const int rg = ensure_splitk(ctx, (uint64_t)S * n * M)) return rg;
    StreamArgs a = {};
    a.xs = xs; a.xs_plane = xs_plane; a.ldxs = ldxs; a.groups = 1; a.M = M; a.K = K; a.n = n; a.ldy = M; a.w[0] = wq; a.ws[0] = wsc; a.y[0] = ctx->splitk;
    a.ksplit = S; a.ysplit = (uint64_t)n * M;
    const int rs = wsc ? launch_stream_q8b_maxt(ctx, a, name, maxt, wdt) : launch_stream_b9_maxt(ctx, a, name, maxt);
    if (rs) return rs;
    if (g_prepare_only) return 0;
    StreamReduceArgs r = {};
    r.part = ctx->splitk; r.stride = a.ysplit; r.resid = resid; r.y = y; r.gamma = gamma; r.h = h; r.S = S; r.d = M; r.ldy = M; r.hs = hs; r.hs_plane = hs_plane;
    { TraceScope ts_(ctx->stream, "stream_reduce_norm"); LH_LAUNCH(k_stream_reduce_norm, dim3(n), dim3(256), 0, ctx->stream, r); }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// fp32 weights, long prompts: the exact bf16 x 9 GEMM (kernels_gemm_b9.h) - 128 x 256 tiles, eight waves, X split into planes by one pass in
// front (n K 10 bytes through HBM: ~1 % of the GEMM it feeds).  Per tile area one slab takes 0.62 (a partly filled round) to 0.73 (every CU
// busy: the chip is then power-bound and clocks down) of k_gemm_glds' time, but the tiles are large: gemm_mfma_group takes it where rounds x slab
// time beats the fp32 kernel's best shape.  13B at 1024 rows inside the model (profiles/r05_p13_kernel_trace.txt): wq|wk|wv 1040 us against
// 1407, w1|w3 2030 against 2380, w2 1100 against 1290-1525, wo 424 against 450 (160 tiles of 128 x 256 against 256 of 128 x 160).
static bool gemm_b9_ok(const GemmArgs& a) {
    return a.N > 128 && !a.causal && a.splits <= 1 && gemm_dma_ok(a) && a.K >= 16 * GBK && a.K % 8 == 0;
}
// wdt = 1: a.w[] are the halves of an f16 model (k_gemm_b9_h, kernels_gemm_f16.h) - the same tiles, split count, k_split3_rows in front and reduce pass
// behind; the ring depth is the half kernel's own and no part of the sums.  Its stage is 40 KB, so three fit: synthetic 7B, one Eval of 193 / 512 / 1024
// tokens 19.5 / 38.6 / 69.4 ms with three stages against 20.2 / 39.1 / 69.3 with two (-DB9H_NST=2; profiles/f16_tiles.txt) - three ship.
// -DB9H_PRODUCTS=8 issues the two products of the weights' zero plane as well (the fallback, had six not been byte-equal on the GPU).
#ifndef B9H_NST
#define B9H_NST 3
#endif
#ifndef B9H_PRODUCTS
#define B9H_PRODUCTS 6
#endif
static int launch_gemm_b9(lh_ctx* ctx, GemmArgs a, const char* name, uint32_t splits, int wdt = 0) {
    auto kern = k_gemm_b9<1, 8, 4, 1, 2>;
    auto kern_h = k_gemm_b9_h<1, 8, 4, 1, B9H_NST, B9H_PRODUCTS>;
    const size_t lds = wdt == 1 ? gemm_b9_h_lds_bytes(B9H_NST) : 2 * gemm_b9_stage_bytes(128, 256);
    static bool flags[16] = {}, flags_h[16] = {};
    int rc = wdt == 1 ? set_lds_once(ctx, kern_h, lds, flags_h) : set_lds_once(ctx, kern, lds, flags);
    if (rc) return rc;
    if (!ensure_xs3(ctx, (uint64_t)3 * a.N * a.K)) LH_FAIL(ctx, LH_ENOMEM, "%s: planes of %u x %u activations", name, a.N, a.K);
    a.xs = ctx->xs3; a.xs_plane = (uint64_t)a.N * a.K; a.ldxs = a.K;
    a.splits = splits > 1 ? splits : 0; a.part = nullptr;
    if (splits > 1) {
        if ((rc = ensure_splitk(ctx, (uint64_t)a.groups * splits * a.N * a.M))) return rc;
        a.part = ctx->splitk;
    }
    if (g_prepare_only) return 0;
    {
        TraceScope ts_(ctx->stream, "split3_rows");
        Split3Args sa = {a.x, ctx->xs3, a.xs_plane, a.K, a.ldx, a.K};
        LH_TRACE("k_split3_rows");
        LH_LAUNCH(k_split3_rows, dim3(a.N), dim3(256), 0, ctx->stream, sa);
    }
    const uint64_t items = (uint64_t)((a.N + 127) / 128) * ((a.M + 255) / 256) * a.groups * (splits > 1 ? splits : 1);
    ProfScope ps(ctx->stream, name, (uint64_t)a.M * a.K * (wdt == 1 ? 2 : 4) * a.groups);
    if (wdt == 1) {
        LH_TRACE("k_gemm_b9_h<1,8,4,1,%d>/s%u", B9H_NST, splits > 1 ? splits : 1u);
        LH_LAUNCH_AS("k_gemm_b9_h", kern_h, dim3((uint32_t)std::min<uint64_t>(items, (uint64_t)ctx->ds->num_cu)), dim3(512), lds, ctx->stream, a);
    } else {
        LH_TRACE("k_gemm_b9<1,8,4,1,2>/s%u", splits > 1 ? splits : 1u);
        LH_LAUNCH_AS("k_gemm_b9", kern, dim3((uint32_t)std::min<uint64_t>(items, (uint64_t)ctx->ds->num_cu)), dim3(512), lds, ctx->stream, a);
    }
    if (splits > 1) {
        const uint64_t quads = (uint64_t)a.groups * a.N * (a.M / 4);
        LH_TRACE("k_splitk_reduce");
        LH_LAUNCH(k_splitk_reduce, dim3((uint32_t)std::min<uint64_t>((quads + 255) / 256, 4096)), dim3(256), 0, ctx->stream, a);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// fused != nullptr: GEMM_EPI_SILU_MUL (w = {w1, w3}, y[0] = gated output [n][M]) or GEMM_EPI_QKV_ROPE (w = {wq, wk, wv}; outputs in *fused) in
// the epilogue of the LDS-DMA tile GEMM; returns ST_NA when the launch cannot take it (short prompt, split-K, register-staged kernel) and
// the caller runs the plain GEMM + the separate pass.
// The halves behind fp32 image slots (an f16 plan with lh_ctx_set_f16_stream or lh_ctx_set_f16_tiles on, eval_prefill): w[g] of the launch names the
// image slot of a matrix whose n halves are at half[g] and which is NOT widened yet.  A stream launch reads the halves (k_stream_*_h) if `stream` is set,
// a k_gemm_b9 launch reads them (k_gemm_b9_h) if `tiles` is set; every other launch widens the matrix into its slot first, directly in front of itself
// (HalfSrc::widen: k_widen_f16 per matrix), and reads the image as ever.
struct HalfSrc {
    const float* half[3];
    uint64_t n;
    bool* wide[3];   // the caller's "slot holds the matrix" flags
    bool stream, tiles;
    void widen(lh_ctx* ctx, const float* const* w, uint32_t groups) const {
        for (uint32_t g = 0; g < groups; ++g)
            if (!*wide[g]) { widen_f16_launch(ctx, half[g], (float*)w[g], n); *wide[g] = true; }   // (a launch error surfaces at the layer's hipGetLastError)
    }
};
// One launch site of the stream chain over matrices that may still be halves: launch(w, wdt) is the site's gemm_stream_group / gemm_stream_split call.
// hs->stream: the halves as they are.  Otherwise the launch reads the image, which is widened only if the chain HAS a launch for the shape - asked with
// a prepare-only pass, which enqueues nothing - so that a widening pass never stands in front of a launch that does not read it.
template <typename F>
static int stream_src(lh_ctx* ctx, const HalfSrc* hs, const float* const* w, uint32_t groups, F&& launch) {
    if (!hs) return launch(w, 0);
    if (hs->stream) return launch(hs->half, 1);
    const bool was = g_prepare_only;
    g_prepare_only = true;
    const int rs = launch(w, 0);
    g_prepare_only = was;
    if (rs || was) return rs;
    hs->widen(ctx, w, groups);
    return launch(w, 0);
}
int gemm_mfma_group(lh_ctx* ctx, const float* x, uint32_t ldx, uint32_t groups, const float* const* w, float* const* y, const float* const* r, uint32_t M,
                    uint32_t K, uint32_t n, uint32_t ldy, const char* name, const GemmArgs* fused = nullptr, bool split_ok = true, const HalfSrc* hs = nullptr) {
    if (n <= stream_max_rows() && !fused) {
        const int rs = stream_src(ctx, hs, w, groups, [&](const float* const* ws, int wdt) { return gemm_stream_group(ctx, x, ldx, groups, ws, y, r, M, K, n, ldy, name, nullptr, wdt); });
        if (rs != ST_NA) return rs;
    }
    // (hs: every decision below is taken on the image slots' addresses, the widened twin's; the matrices are widened directly in front of the launch chosen -
    // or not at all where it is k_gemm_b9 and the halves may be read)
    auto wide = [&]() { if (hs) hs->widen(ctx, w, groups); };
    GemmArgs a = {};
    if (fused) a = *fused;
    a.x = x; a.groups = groups; a.N = n; a.M = M; a.K = K; a.ldx = ldx; a.ldy = ldy;
    for (uint32_t g = 0; g < groups; ++g) { a.w[g] = w[g]; a.y[g] = y ? y[g] : nullptr; a.r[g] = r ? r[g] : nullptr; }
    if (fused && fused->epi == GEMM_EPI_SILU_MUL) { a.groups = 1; a.M = 2 * M; }   // one matrix of 2 M virtual rows (w1, w3 interleaved)
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, tn = (n + 127) / 128;
    // tile width and split-K chosen together: slab times of the busiest CU (pick_splitk) x tile width x the narrow tiles' lower matrix-pipe yield
    const bool may_split = !fused && a.K >= 16 * GBK && gemm_dma_ok(a) && a.M % 4 == 0 && ldy % 4 == 0;
    auto cost = [&](uint32_t bm, double penalty) {
        const uint32_t tiles = tn * ((a.M + bm - 1) / bm) * a.groups;
        double c = (double)((tiles + ncu - 1) / ncu) * (a.K / GBK + 8) * bm;
        if (may_split) pick_splitk(tiles, ncu, a.K / GBK, 128, bm, (uint64_t)a.groups * n * a.M, &c);
        return c * penalty;
    };
    if (fused) {
        // only where the epilogue exists: the DMA kernel, whole contraction per tile (no split-K: at least one tile per CU), long prompts
        if (n <= 64 || !gemm_dma_ok(a) || a.K < 16 * GBK || tn * ((a.M + 159) / 160) * a.groups < ncu) return ST_NA;
        if (fused->epi == GEMM_EPI_QKV_ROPE && (fused->hd % 2 || M % fused->hd)) return ST_NA;
    }
    // up to 64 rows: 64 x 128 tiles (half the matrix work of a 128-row tile whose upper half would be padding)
    if (n <= 64) { wide(); return launch_gemm<2, 2, 1, 2>(ctx, a, name); }
    const double c128 = cost(128, 1.0), c160 = cost(160, 1.03), c64 = cost(64, 1.10);
    if (split_ok && gemm_b9_ok(a)) {
        const uint64_t tiles9 = (uint64_t)tn * ((a.M + 255) / 256) * a.groups;
        const uint32_t nkf = a.K / GBK;
        const double unit = may_split ? 2.0 * 128 * GBK / (157.3e6 / 256.0) : 1.0;      // cost() is in microseconds when split-K is on the table
        constexpr double B9_SLAB = 0.56;   // a 128 x 256 slab of k_gemm_b9 in units of k_gemm_glds' 128 x 128 slab per tile row (0.62 with nine products, r05; eight: x 8 / 9 measured -9.5 %)
        double c9 = (double)((tiles9 + ncu - 1) / ncu) * (nkf + 8) * 256 * B9_SLAB * unit;
        uint32_t s9 = 1;
        if (may_split)      // (cost in microseconds: the reduce pass as in pick_splitk)
            for (uint32_t s2 = 2; s2 <= 8; ++s2) {
                if (nkf / s2 < 16) break;
                const double c = (double)((tiles9 * s2 + ncu - 1) / ncu) * ((nkf + s2 - 1) / s2 + 8) * 256 * B9_SLAB * unit + (double)(s2 + 1) * a.groups * n * a.M * 4.0 / 4e6 + 5.0;
                if (c < c9 * 0.95) { c9 = c; s9 = s2; }
            }
        if (c9 < 0.97 * std::min(c128, std::min(c160, c64))) {
            bool halves = hs && hs->tiles && !a.ldw;
            for (uint32_t g = 0; halves && g < groups; ++g) halves = ((uintptr_t)hs->half[g] & 15) == 0;
            if (halves) {
                for (uint32_t g = 0; g < groups; ++g) a.w[g] = hs->half[g];
                return launch_gemm_b9(ctx, a, name, s9, 1);
            }
            wide();
            return launch_gemm_b9(ctx, a, name, s9);
        }
    }
    wide();
    if (c160 < c128 && c160 <= c64) return launch_gemm<4, 1, 1, 5>(ctx, a, name);
    if (c64 < c128) return launch_gemm<2, 2, 2, 1>(ctx, a, name);
    return launch_gemm<2, 2, 2, 2>(ctx, a, name);
}

static int gemm_mfma(lh_ctx* ctx, const float* w, const float* x, float* y, const float* resid, uint32_t M, uint32_t K, uint32_t n, uint32_t ldx,
                     uint32_t ldy, const char* name, bool split_ok, const HalfSrc* hs = nullptr) {
    return gemm_mfma_group(ctx, x, ldx, 1, &w, &y, resid ? &resid : nullptr, M, K, n, ldy, name, nullptr, split_ok, hs);
}

// Y[n][M] = X[n][K] . W[M][K]^T (+ resid).  N >= 32: fp32 MFMA GEMM (compute-bound side); smaller N: the weight-streaming
// kernel with NC activation rows in registers (HBM-bound side, weights read once per NC rows).
static constexpr uint32_t MFMA_MIN_ROWS = 9;
// block-int8: below this many tokens single-token steps on the int8 stream (2.1 ms each on 7B) beat the dequantising GEMM
static constexpr uint32_t Q8_GEMM_MIN_ROWS = 9;
// split_ok = false: the operands may hold values outside split_exact_values' range (common.h) - no launch on the bf16-split GEMM
static int gemm_small_n_src(lh_ctx* ctx, const float* w, const float* x, float* y, const float* resid, uint32_t M, uint32_t K, uint32_t n,
                            uint32_t ldx, uint32_t ldy, const char* name, bool split_ok, const HalfSrc* hs);
int gemm_small_n(lh_ctx* ctx, const float* w, const float* x, float* y, const float* resid, uint32_t M, uint32_t K, uint32_t n,
                 uint32_t ldx, uint32_t ldy, const char* name, bool split_ok = true) {
    return gemm_small_n_src(ctx, w, x, y, resid, M, K, n, ldx, ldy, name, split_ok, nullptr);
}
// hs: see HalfSrc (w is then the image slot of a matrix that is not widened yet)
static int gemm_small_n_src(lh_ctx* ctx, const float* w, const float* x, float* y, const float* resid, uint32_t M, uint32_t K, uint32_t n,
                            uint32_t ldx, uint32_t ldy, const char* name, bool split_ok, const HalfSrc* hs) {
    if (K % 4) LH_FAIL(ctx, LH_ESHAPE, "gemm %s: K=%u must be a multiple of 4", name, K);
    // from 9 rows on the MFMA GEMM (64-row tiles, split-K) beats two or more passes of the 8-column weight stream (7B, one Eval:
    // 8 rows 10.0 ms and 16 rows 18.4 ms on the stream; 17 rows 11.1 ms on the MFMA path)
    if (n >= MFMA_MIN_ROWS && K % GBK == 0 && ldx % 4 == 0) return gemm_mfma(ctx, w, x, y, resid, M, K, n, ldx, ldy, name, split_ok, hs);
    if (n >= 2) {   // 2..8 rows on the general path: the streaming MFMA kernel
        const int rs = stream_src(ctx, hs, &w, 1, [&](const float* const* ws, int wdt) { return gemm_stream_group(ctx, x, ldx, 1, ws, &y, resid ? &resid : nullptr, M, K, n, ldy, name, nullptr, wdt); });
        if (rs != ST_NA) return rs;
    }
    if (hs) hs->widen(ctx, &w, 1);
    const uint32_t K4 = K / 4;
    const int ki = (int)((K4 + TH - 1) / TH);
    // activation columns per pass: what fits the 128 registers of a 1024-thread workgroup without scratch (ISA-checked per instantiation)
    const uint32_t NCmax = ki <= 2 ? 8 : (ki <= 4 ? 4 : 2);
    for (uint32_t c0 = 0; c0 < n; c0 += NCmax) {
        GemmColsArgs a;
        a.w = w; a.x = x + (size_t)c0 * ldx; a.y = y + (size_t)c0 * ldy; a.resid = resid ? resid + (size_t)c0 * ldy : nullptr;
        a.M = M; a.K = K; a.ldx = ldx; a.ldy = ldy; a.ncols = std::min(NCmax, n - c0);
        int rc;
        switch (ki) {
            case 1: rc = launch_cols<1, 2, 8>(ctx, a, name); break;
            case 2: rc = launch_cols<2, 2, 8>(ctx, a, name); break;
            case 3: rc = launch_cols<3, 2, 4>(ctx, a, name); break;
            case 4: rc = launch_cols<4, 1, 4>(ctx, a, name); break;
            case 5: rc = launch_cols<5, 1, 2>(ctx, a, name); break;
            case 6: rc = launch_cols<6, 1, 2>(ctx, a, name); break;
            default: LH_FAIL(ctx, LH_EUNSUPPORTED, "gemm %s: K=%u exceeds the supported 24576 columns", name, K);
        }
        if (rc) return rc;
    }
    return 0;
}

// ---- short prompts (2..8 token rows, fp32 weights): one fused pass over the weights per matrix group (kernels_skinny.h) -------
static constexpr uint32_t SKINNY_NP = 8, SKINNY_KC_MAX = 4096;
// shapes the kernel is built for: every contraction length a whole number of ring groups (256 floats), RoPE pairs inside a head
// whole-model check for the streaming MFMA kernel (the 2..8-row prompts prefer it over k_skinny: 6.0 vs 6.5 ms on 7B)
static bool stream_shape_ok(lh_ctx* ctx, const ModelDesc& m) {
    if (m.wtype != 0 || m.d % 128 || m.F % 128) return false;
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu;
    auto maxt = [&](uint32_t rows) { return (rows / 16 + ncu - 1) / ncu; };
    return maxt(3 * m.d) <= 8 && maxt(2 * m.F) <= 8;
}
static bool skinny_ok(const ModelDesc& m, uint32_t n) {
    return m.wtype == 0 && n >= 2 && n <= SKINNY_NP && m.d % SK_GRP == 0 && m.F % SK_GRP == 0 && m.hd % 2 == 0;
}
template <int PRO, int EPI, int MAP>
static int launch_skinny(Plan* p, SkinnyArgs a, const char* name) {
    lh_ctx* ctx = p->ctx;
    auto kern = k_skinny<SKINNY_NP, PRO, EPI, MAP>;
    // K-chunks: the staged activation tile is at most 8 x 4096 floats; chunks are whole ring groups (256 floats) of nearly equal length
    constexpr uint32_t GR = SK_GRP;
    const uint32_t nchunks = (a.K + SKINNY_KC_MAX - 1) / SKINNY_KC_MAX;
    const uint32_t kc_max = ((a.K / GR + nchunks - 1) / nchunks) * GR;
    const uint32_t nwg = (uint32_t)ctx->ds->num_cu, npairs = a.M / 2;
    a.rows_cap = 2 * ((npairs + nwg - 1) / nwg) + 2;
    const size_t lds = skinny_lds_bytes(SKINNY_NP, kc_max, a.rows_cap, a.hd, EPI == EPI_RESID, nchunks > 1, EPI == EPI_QKV_ROPE);
    if (lds > 160 * 1024) LH_FAIL(ctx, LH_EUNSUPPORTED, "skinny %s: %zu bytes of LDS needed", name, lds);
    static bool flags[16] = {};
    int rc0 = set_lds_once(ctx, kern, 160 * 1024, flags);
    if (rc0) return rc0;
    if (g_prepare_only) return 0;
    if (nchunks > 1 && (rc0 = grow_floats(ctx, &p->part, &p->part_cap, (uint64_t)SKINNY_NP * a.M))) return rc0;
    ProfScope ps(ctx->stream, name, (uint64_t)a.M * a.K * 4);
    uint32_t k0 = 0;
    for (uint32_t ch = 0; ch < nchunks; ++ch) {
        const uint32_t kc = std::min(kc_max, a.K - k0);
        SkinnyArgs b = a;
        b.k0 = k0; b.kc = kc;
        b.part_in = ch > 0 ? p->part : nullptr;
        b.part_out = ch + 1 < nchunks ? p->part : nullptr;
        LH_LAUNCH_AS("k_skinny", kern, dim3(nwg), dim3(SK_TH), lds, ctx->stream, b);
        k0 += kc;
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

static int launch_attention(lh_ctx* ctx, const AttnArgs& a, uint32_t max_T) {
    if (a.hd > ATT_TH || ATT_TH % a.hd || a.hd % 4) LH_FAIL(ctx, LH_EUNSUPPORTED, "attention: head dim %u unsupported (needs to divide %d)", a.hd, ATT_TH);
    const size_t lds = (2 * (size_t)((max_T + 63) & ~63u) + ATT_TH) * 4;
    static bool flags[16] = {};
    static size_t cur[16] = {};
    if (lds > 48 * 1024 && lds > cur[ctx->device & 15]) {
        flags[ctx->device & 15] = false;
        int rc = set_lds_once(ctx, k_attention, 160 * 1024, flags);
        if (rc) return rc;
        cur[ctx->device & 15] = 160 * 1024;
    }
    if (lds > 160 * 1024) LH_FAIL(ctx, LH_EUNSUPPORTED, "attention: %u keys exceed the single-pass LDS budget", max_T);
    if (g_prepare_only) return 0;
    if (g_only) return 0;
    ProfScope ps(ctx->stream, "attention", (uint64_t)2 * max_T * a.d * 4);
    LH_TRACE("k_attention%s/hd%u/n%u", a.rows ? "/rows" : "", a.hd, a.n);
    LH_LAUNCH(k_attention, dim3(a.d / a.hd, a.n), dim3(ATT_TH), lds, ctx->stream, a);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// decode attention for long-context plans: chunks of ATT_TC keys per workgroup + combine
// (part: [rows][H][chunks][hd + 2] partials; rows = a.n query rows of a batched Eval, 1 otherwise)
static int launch_attention_split(Plan* p, const AttnArgs& a, float* part) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (a.hd != 128) LH_FAIL(ctx, LH_EUNSUPPORTED, "split attention: head dim %u", a.hd);
    const uint32_t nch = (m.ctx + ATT_TC - 1) / ATT_TC, nrows = a.rows ? a.n : 1u;
    if (g_prepare_only || g_only) return 0;
    {
        ProfScope ps(ctx->stream, "attention_split", (uint64_t)2 * m.ctx * a.d * 4 * nrows);
        LH_TRACE("k_attention_split%s/c%u/n%u", a.rows ? "/rows" : "", nch, nrows);
        LH_LAUNCH(k_attention_split, dim3(m.H, nch, nrows), dim3(ATT_TH), 0, ctx->stream, a, part);
    }
    {
        ProfScope ps(ctx->stream, "attention_combine", (uint64_t)m.H * nch * (a.hd + 2) * 4 * nrows);
        LH_TRACE("k_attention_combine/c%u/n%u", nch, nrows);
        LH_LAUNCH(k_attention_combine, dim3(m.H, nrows), dim3(128), 0, ctx->stream, a, (const float*)part, nch);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// lh_batch_feed: blocks of query rows that share a cache (kernels_attn_seg.h).  QB = rows per block the schedule was cut for (2, 4, 8); the blocks of ONE
// row at the head of the table (decode rows) take the QB = 1 instantiation: with the registers of QB queries the kernels fit one workgroup per CU, with one
// query two, like the per-row kernels - 32 decode rows behind 1000 keys ran 322 us per layer on the QB = 8 build against 174 us row by row
// (profiles/feed_ragged.txt).
template <int QB>
static int launch_attention_seg_blocks(Plan* p, const AttnArgs& a, const BatchCtx* bc, const AttnBlock* blocks, uint32_t n_blocks) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (!n_blocks) return 0;
    if (bc->attn_part) {
        const uint32_t nch = (m.ctx + ATT_TC - 1) / ATT_TC, nch_pass = (bc->max_T + ATT_TC - 1) / ATT_TC;
        ProfScope ps(ctx->stream, "attention_split_seg", (uint64_t)2 * bc->max_T * a.d * 4 * n_blocks);
        LH_TRACE("k_attention_split_seg/c%u/qb%u/n%u", nch_pass, (uint32_t)QB, a.n);
        LH_LAUNCH_AS("k_attention_split_seg", k_attention_split_seg<QB>, dim3(m.H, nch_pass, n_blocks), dim3(ATT_TH), 0, ctx->stream, a, blocks, bc->attn_part, nch);
        return 0;
    }
    const uint32_t Tp = (bc->max_T + 63) & ~63u;
    const size_t lds = ((size_t)2 * QB * Tp + (size_t)QB * ATT_TH) * 4;
    ProfScope ps(ctx->stream, "attention_seg", (uint64_t)2 * bc->max_T * a.d * 4 * n_blocks);
    LH_TRACE("k_attention_seg/hd%u/qb%u/n%u", a.hd, (uint32_t)QB, a.n);
    LH_LAUNCH_AS("k_attention_seg", k_attention_seg<QB>, dim3(a.d / a.hd, n_blocks), dim3(ATT_TH), lds, ctx->stream, a, blocks, Tp);
    return 0;
}
template <int QB>
static int launch_attention_seg_qb(Plan* p, const AttnArgs& a, const BatchCtx* bc) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (g_prepare_only || g_only) return 0;
    if (bc->attn_part && a.hd != 128) LH_FAIL(ctx, LH_EUNSUPPORTED, "split attention: head dim %u", a.hd);
    int rc;
    if ((rc = launch_attention_seg_blocks<1>(p, a, bc, bc->blocks, bc->n_blocks1))) return rc;
    if ((rc = launch_attention_seg_blocks<QB>(p, a, bc, bc->blocks + bc->n_blocks1, bc->n_blocks - bc->n_blocks1))) return rc;
    if (bc->attn_part) {
        const uint32_t nch = (m.ctx + ATT_TC - 1) / ATT_TC;
        ProfScope ps(ctx->stream, "attention_combine", (uint64_t)m.H * nch * (a.hd + 2) * 4 * a.n);
        LH_TRACE("k_attention_combine/c%u/n%u", nch, a.n);
        LH_LAUNCH(k_attention_combine, dim3(m.H, a.n), dim3(128), 0, ctx->stream, a, (const float*)bc->attn_part, nch);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
static constexpr size_t ATT_SEG_LDS_MAX = 48 * 1024;   // the single-pass segment kernel stays inside the LDS a launch gets without an attribute
static bool attention_seg_fits(uint32_t qb, uint32_t max_T) { return ((size_t)2 * qb * ((max_T + 63) & ~63u) + (size_t)qb * ATT_TH) * 4 <= ATT_SEG_LDS_MAX; }

// a tick whose pods share a prompt prefix (lh_batch_fork; kernels_attn_share.h): k_attention_split's grid, the full chunks inside a group's prefix read
// once per block of up to QB member rows.  The same partial records at the same addresses, so the combine is launch_attention_split's.
template <int QB>
static int launch_attention_split_shared(Plan* p, const AttnArgs& a, const BatchCtx* bc) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (a.hd != 128) LH_FAIL(ctx, LH_EUNSUPPORTED, "split attention: head dim %u", a.hd);
    if (a.n > SHARE_ROWS_MAX) LH_FAIL(ctx, LH_EINVAL, "shared attention: %u rows (the table holds %u)", a.n, SHARE_ROWS_MAX);
    const uint32_t nch = (m.ctx + ATT_TC - 1) / ATT_TC;
    if (g_prepare_only || g_only) return 0;
    {
        ProfScope ps(ctx->stream, "attention_split_shared", (uint64_t)2 * m.ctx * a.d * 4 * a.n);
        LH_TRACE("k_attention_split_shared/c%u/qb%u/b%u/n%u", nch, (uint32_t)QB, bc->share_blocks, bc->share_rows);
        LH_LAUNCH_AS("k_attention_split_shared", k_attention_split_shared<QB>, dim3(m.H, nch, a.n), dim3(ATT_TH), 0, ctx->stream, a, bc->share, bc->attn_part);
    }
    {
        ProfScope ps(ctx->stream, "attention_combine", (uint64_t)m.H * nch * (a.hd + 2) * 4 * a.n);
        LH_TRACE("k_attention_combine/c%u/n%u", nch, a.n);
        LH_LAUNCH(k_attention_combine, dim3(m.H, a.n), dim3(128), 0, ctx->stream, a, (const float*)bc->attn_part, nch);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// the attention of a batched Eval's rows: query blocks (a feed), else row by row (ticks; LLAMAHIP_FEED_ROW_ATTN)
static int launch_attention_rows(Plan* p, const AttnArgs& a, const BatchCtx* bc) {
    lh_ctx* ctx = p->ctx;
    if (bc->share && bc->attn_part) {
        switch (bc->share_qb) {
            case 2: return launch_attention_split_shared<2>(p, a, bc);
            case 4: return launch_attention_split_shared<4>(p, a, bc);
            case 8: return launch_attention_split_shared<8>(p, a, bc);
            default: LH_FAIL(ctx, LH_EINVAL, "shared attention: blocks of %u rows (2, 4 or 8)", bc->share_qb);
        }
    }
    if (bc->blocks) {
        if (a.hd > ATT_TH || ATT_TH % a.hd || a.hd % 4) LH_FAIL(ctx, LH_EUNSUPPORTED, "attention: head dim %u unsupported (needs to divide %d)", a.hd, ATT_TH);
        // (a single pass whose score rows outgrow the LDS budget - wide blocks on a head size without the split kernel - keeps the per-row kernel)
        if (bc->attn_part || attention_seg_fits(bc->qb, bc->max_T)) {
            switch (bc->qb) {
                case 2: return launch_attention_seg_qb<2>(p, a, bc);
                case 4: return launch_attention_seg_qb<4>(p, a, bc);
                case 8: return launch_attention_seg_qb<8>(p, a, bc);
                default: LH_FAIL(ctx, LH_EINVAL, "segment attention: blocks of %u rows (2, 4 or 8)", bc->qb);
            }
        }
    }
    if (bc->blocks) LH_TRACE("feed_attention_fallback/rows/qb%u/T%u", bc->qb, bc->max_T);   // (so that an A/B on such a shape shows what it compared)
    if (bc->attn_part) return launch_attention_split(p, a, bc->attn_part);
    return launch_attention(ctx, a, p->md.ctx);
}

// ---------------------------------------------------------------------------------------------------
static void spec_free(Plan* p);
int plan_ensure_rows(Plan* p, uint32_t n) {
    if (n <= p->n_cap) return 0;
    lh_ctx* ctx = p->ctx;
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const ModelDesc& m = p->md;
    auto re = [&](float** ptr, size_t nfloats) -> int {
        if (*ptr) LH_HIP(ctx, hipFree(*ptr));
        *ptr = nullptr;
        LH_HIP(ctx, hipMalloc((void**)ptr, nfloats * 4));
        return 0;
    };
    const size_t nd = (size_t)n * m.d, nf = (size_t)n * m.F;
    int rc = 0;
    rc |= re(&p->xa, nd); rc |= re(&p->xb, nd); rc |= re(&p->h, nd); rc |= re(&p->q, nd); rc |= re(&p->attn, nd); rc |= re(&p->g, nf);
    if (n > 1) { rc |= re(&p->qraw, nd); rc |= re(&p->kraw, nd); rc |= re(&p->vraw, nd); rc |= re(&p->a1, nf); rc |= re(&p->a3, nf); }
    if (m.last_stage()) rc |= re(&p->logits, (size_t)n * m.V);
    if (rc) return LH_EHIP;
    if (n > 1 && (m.wtype == 7 || m.wtype == 0 || m.wtype == 1 || m.wtype == 2)) {   // the activations as planes: every row of a block-int8 plan, up to k_stream_b9's 64 rows of an fp32 one (f16: the fp32 schedule; block-int4: the int8 one)
        if (p->s3) LH_HIP(ctx, hipFree(p->s3));
        p->s3 = nullptr;
        p->s3_rows = m.wtype == 7 || m.wtype == 2 ? n : std::min<uint32_t>(n, B9S_MAX_ROWS);
        LH_HIP(ctx, hipMalloc((void**)&p->s3, (size_t)3 * p->s3_rows * (2 * (size_t)m.d + m.F) * 2));
    }
    if (p->tokens_dev) LH_HIP(ctx, hipFree(p->tokens_dev));
    LH_HIP(ctx, hipMalloc((void**)&p->tokens_dev, (size_t)n * 4));
    p->n_cap = n;
    p->scratch_gen++;
    return 0;
}

static constexpr uint32_t SP_SLOTS = 64;

int plan_create(lh_ctx* ctx, const ModelDesc& md, Plan** out) {
    if (md.d % md.H || md.d % 4 || md.F % 4) LH_FAIL(ctx, LH_ESHAPE, "plan: embd %u / heads %u / ff %u not supported", md.d, md.H, md.F);
    Plan* p = new Plan();
    p->ctx = ctx;
    p->md = md;
    const char* env = getenv("LLAMAHIP_NO_GRAPH");
    p->use_graph = !(env && env[0] == '1');
    int rc = ensure_rope_table(ctx, md.ctx, md.hd, &p->rope);
    if (rc) { delete p; return rc; }
    hipError_t e = hipMalloc((void**)&p->sp_dev, sizeof(StepParams) * SP_SLOTS);
    if (e == hipSuccess) e = hipHostMalloc((void**)&p->sp_host, sizeof(StepParams) * SP_SLOTS, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&p->argmax_dev, 4);
    if (e != hipSuccess) { set_error(ctx, "plan_create: %s", hipGetErrorString(e)); plan_destroy(p); return LH_ENOMEM; }
    rc = plan_ensure_rows(p, 1);
    if (rc) { plan_destroy(p); return rc; }
    if (md.wtype == 1) {   // the fp32 images of the widened routes (Plan::md_wide): sized here, once
        const uint64_t d = md.d, F = md.F;
        if ((rc = wide_image(ctx, 4 * d * d + 3 * d * F, 4, 0, &p->wide_layer)) || (md.last_stage() && (rc = wide_image(ctx, (uint64_t)md.V * d, 4, 1, &p->wide_out)))) { plan_destroy(p); return rc; }
        p->md_wide = md;
        p->md_wide.wtype = 0;
        p->md_wide.output = p->wide_out;
        float* w = p->wide_layer;
        for (uint32_t il = md.layer0; il < md.layer1; ++il) {
            LayerW& L = p->md_wide.layers[il];
            L.wq = w; L.wk = w + d * d; L.wv = w + 2 * d * d; L.wo = w + 3 * d * d; L.w1 = w + 4 * d * d; L.w3 = w + 4 * d * d + d * F; L.w2 = w + 4 * d * d + 2 * d * F;
        }
    }
    if (md.wtype == 2) {   // block-int4: the int8 images of the expanded routes, sized here, once; the shadow keeps the model's own scale planes (s_*)
        const uint64_t d = md.d, F = md.F;
        if ((rc = wide_image(ctx, 4 * d * d + 3 * d * F, 1, 0, &p->wide_layer)) || (md.last_stage() && (rc = wide_image(ctx, (uint64_t)md.V * d, 1, 1, &p->wide_out)))) { plan_destroy(p); return rc; }
        p->md_wide = md;
        p->md_wide.wtype = 7;
        p->md_wide.output = p->wide_out;
        const char* w = (const char*)p->wide_layer;
        auto at = [&](uint64_t off) { return (const float*)(w + off); };
        for (uint32_t il = md.layer0; il < md.layer1; ++il) {
            LayerW& L = p->md_wide.layers[il];
            L.wq = at(0); L.wk = at(d * d); L.wv = at(2 * d * d); L.wo = at(3 * d * d); L.w1 = at(4 * d * d); L.w3 = at(4 * d * d + d * F); L.w2 = at(4 * d * d + 2 * d * F);
        }
    }
    p->hist =md.kv_hist ? md.kv_hist : std::make_shared<std::vector<uint32_t>>();
    if (p->hist->size() < md.ctx) p->hist->resize(md.ctx, Plan::HIST_UNKNOWN);
    if (md.ctx > 256 && md.hd == 128) {   // long contexts: decode attention split over the keys (k_attention_split)
        const size_t nch = (md.ctx + ATT_TC - 1) / ATT_TC;
        e = hipMalloc((void**)&p->attn_part, (size_t)md.H * nch * (md.hd + 2) * 4);
        if (e != hipSuccess) { set_error(ctx, "plan_create: %s", hipGetErrorString(e)); plan_destroy(p); return LH_ENOMEM; }
    }
    *out = p;
    return 0;
}

void plan_destroy(Plan* p) {
    if (!p) return;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    for (auto& g : p->graphs) g.drop();
    if (p->ss_dev) hipFree(p->ss_dev);
    if (p->ring_dev) hipFree(p->ring_dev);
    float* bufs[] = {p->xa, p->xb, p->h, p->qraw, p->kraw, p->vraw, p->q, p->attn, p->a1, p->a3, p->g, p->logits, p->scores, p->vt, p->part, p->fa_part, p->emb};
    for (float* b : bufs) if (b) hipFree(b);
    if (p->tokens_dev) hipFree(p->tokens_dev);
    if (p->sp_dev) hipFree(p->sp_dev);
    if (p->sp_host) hipHostFree(p->sp_host);
    if (p->out_tokens_dev) hipFree(p->out_tokens_dev);
    if (p->argmax_dev) hipFree(p->argmax_dev);
    if (p->attn_part) hipFree(p->attn_part);
    if (p->s3) hipFree(p->s3);
    if (p->score_dev) hipFree(p->score_dev);
    spec_free(p);
    delete p;
}

Plan* plan_find_or_create(lh_ctx* ctx, const ModelDesc& md, int* rc) {
    for (Plan* p : ctx->plans)
        if (p->md.same(md)) {
            // same addresses, possibly a NEW cache buffer at a recycled address: the history is the buffer's, not the plan's
            if (md.kv_hist && p->hist != md.kv_hist) { p->hist = md.kv_hist; if (p->hist->size() < md.ctx) p->hist->resize(md.ctx, Plan::HIST_UNKNOWN); }
            *rc = 0;
            return p;
        }
    Plan* p = nullptr;
    *rc = plan_create(ctx, md, &p);
    if (*rc) return nullptr;
    ctx->plans.push_back(p);
    return p;
}

void destroy_plans(lh_ctx* ctx) {
    for (Plan* p : ctx->plans) plan_destroy(p);
    ctx->plans.clear();
}

// ---- decode step (N = 1): 5 kernels per layer --------------------------------------------------------
// advance: 0 = logits only, 1 = greedy argmax + loop bookkeeping, 2 = device sampler + loop bookkeeping
static int enqueue_decode(Plan* p, const StepParams* sp, const float* x_in, float* x_out, int argmax_advance, uint32_t* argmax_out,
                          const uint32_t* tokens_dev = nullptr, uint32_t logits_row = 0) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    const double2* rope = p->rope;
    int rc;
    const float* x = p->xa;
    if (m.first_stage()) {
        if (!g_prepare_only && !g_only) {
            ProfScope ps(ctx->stream, "embed", (uint64_t)m.d * 4);
            TraceScope ts_(ctx->stream, "embed1");
            LH_LAUNCH(k_embed, dim3(1), dim3(256), 0, ctx->stream, m.tok_emb, tokens_dev, sp, p->xa, m.d, m.V);
            LH_HIP(ctx, hipGetLastError());
        }
    } else {
        x = x_in;  // residual stream received from the previous stage
    }
    float* xa = p->xa;
    float* xb = p->xb;
    const float scale = (float)(1.0 / sqrt((double)m.d / (double)m.H));  // llama.go:306
    for (uint32_t il = m.layer0; il < m.layer1; ++il) {
        const LayerW& L = m.layers[il];
        const size_t slot = (size_t)(il - m.cache_layer0) * m.ctx * m.d;
        {   // RMSNorm*gamma -> wq|wk|wv -> RoPE(Q, new K) -> K,V appended to the cache   (llama.go:255-297)
            GemvArgs a = {};
            a.w[0] = L.wq; a.w[1] = L.wk; a.w[2] = L.wv; a.ws[0] = L.s_wq; a.ws[1] = L.s_wk; a.ws[2] = L.s_wv; a.rows_per_mat = m.d; a.M = 3 * m.d; a.K = m.d;
            a.x = x; a.gamma = L.attn_norm; a.q_out = p->q; a.k_cache = m.kc + slot; a.v_cache = m.vc + slot;
            a.rope = rope; a.hd = m.hd; a.d = m.d; a.sp = sp;
            if ((rc = gemv<PRO_RMSNORM, EPI_QKV_ROPE, MAP_BLOCK>(ctx, a, "gemv_qkv_rope", m.wtype))) return rc;
        }
        {   // scores, scale, mask, softmax, PV, head merge   (llama.go:300-333)
            AttnArgs a = {};
            a.q = p->q; a.k_cache = m.kc + slot; a.v_cache = m.vc + slot; a.out = p->attn; a.d = m.d; a.hd = m.hd; a.n = 1; a.scale = scale; a.sp = sp;
            if (p->attn_part) { if ((rc = launch_attention_split(p, a, p->attn_part))) return rc; }
            else if ((rc = launch_attention(ctx, a, m.ctx))) return rc;
        }
        {   // wo + residual   (llama.go:336-340)
            GemvArgs a = {};
            a.w[0] = L.wo; a.ws[0] = L.s_wo; a.M = m.d; a.K = m.d; a.x = p->attn; a.resid = x; a.y = xb;
            if ((rc = gemv<PRO_PLAIN, EPI_RESID, MAP_SINGLE>(ctx, a, "gemv_wo_resid", m.wtype))) return rc;
        }
        {   // RMSNorm*gamma -> w1|w3 -> silu(w1 h) * (w3 h)   (llama.go:346-361)
            GemvArgs a = {};
            a.w[0] = L.w1; a.w[1] = L.w3; a.ws[0] = L.s_w1; a.ws[1] = L.s_w3; a.M = 2 * m.F; a.K = m.d; a.x = xb; a.gamma = L.ffn_norm; a.y = p->g;
            if ((rc = gemv<PRO_RMSNORM, EPI_SILU_MUL, MAP_PAIR>(ctx, a, "gemv_w1w3_silu", m.wtype))) return rc;
        }
        {   // w2 + residual   (llama.go:363-366)
            const bool last = il + 1 == m.layer1;
            GemvArgs a = {};
            a.w[0] = L.w2; a.ws[0] = L.s_w2; a.M = m.d; a.K = m.F; a.x = p->g; a.resid = xb;
            a.y = (last && !m.last_stage()) ? x_out : xa;
            if ((rc = gemv<PRO_PLAIN, EPI_RESID, MAP_SINGLE>(ctx, a, "gemv_w2_resid", m.wtype))) return rc;
        }
        x = xa;
    }
    if (m.last_stage()) {   // final RMSNorm*gamma -> lm_head   (llama.go:374-384)
        {
            GemvArgs a = {};
            a.w[0] = m.output; a.ws[0] = m.s_output; a.M = m.V; a.K = m.d; a.x = x; a.gamma = m.norm; a.y = p->logits + logits_row * (size_t)m.V;
            if ((rc = gemv<PRO_RMSNORM, EPI_STORE, MAP_SINGLE>(ctx, a, "gemv_lmhead", m.wtype))) return rc;
        }
        if (g_only) {
        } else if (argmax_advance == 2 && !g_prepare_only) {
            ProfScope ps(ctx->stream, "sample", (uint64_t)m.V * 4);
            TraceScope ts_(ctx->stream, "sample");
            if ((rc = sample_launch(ctx, p->logits, m.V, p->ss_dev, p->ring_dev, (StepParams*)sp, p->out_tokens_dev, argmax_out, nullptr, nullptr, nullptr, 1, p->smp_topk))) return rc;
        } else if ((argmax_advance || argmax_out) && !g_prepare_only) {
            ProfScope ps(ctx->stream, "argmax", (uint64_t)m.V * 4);
            TraceScope ts_(ctx->stream, "argmax");
            LH_LAUNCH(k_argmax_advance, dim3(1), dim3(1024), 0, ctx->stream, (const float*)p->logits, m.V, (StepParams*)sp, p->out_tokens_dev,
                               argmax_out, argmax_advance ? 1 : 0);
            LH_HIP(ctx, hipGetLastError());
        }
    }
    return 0;
}

static int ensure_out_tokens(Plan* p, uint32_t n) { return grow(p->ctx, &p->out_tokens_dev, &p->out_cap, n, 4, 4096, &p->out_gen); }

// slot: Plan::G_*; the multi-step slots capture GRAPH_MULTI consecutive steps (the step parameters advance in device memory).  The slots never run
// eagerly: a prepare-only pass in front of the capture sets the kernel attributes and sizes the buffers.
static int ensure_decode_graph(Plan* p, int slot) {
    const int adv = slot == Plan::G_STEP ? 0 : (slot == Plan::G_ADV1 || slot == Plan::G_ADVN) ? 1 : 2;
    const uint32_t reps = (slot == Plan::G_ADVN || slot == Plan::G_SMPN) ? Plan::GRAPH_MULTI : 1;
    int rc;
    if (adv && (rc = ensure_out_tokens(p, 1))) return rc;
    const DecodeKey key = {p->scratch_gen, adv ? p->out_gen : 0, adv == 2 ? p->smp_gen : 0};
    if (p->graphs[slot].current(key)) return 0;
    g_prepare_only = true;
    rc = enqueue_decode(p, p->sp_dev, nullptr, nullptr, adv, nullptr);
    g_prepare_only = false;
    if (rc) return rc;
    return p->graphs[slot].capture(p->ctx, key, "", [&] {
        int r = 0;
        for (uint32_t i = 0; i < reps && !r; ++i) r = enqueue_decode(p, p->sp_dev, nullptr, nullptr, adv, nullptr);
        return r;
    });
}
// n_steps resident steps as graph launches: as many GRAPH_MULTI-step launches as fit, single steps for the rest
static int launch_resident_steps(Plan* p, uint32_t n_steps, int slot1, int slotn) {
    lh_ctx* ctx = p->ctx;
    int rc;
    uint32_t s = 0;
    // both graphs are captured at the first resident call of a context, whatever its length: a short warm-up run then pays for the
    // capture + instantiation of the multi-step graph too, not the first long run after it
    if ((rc = ensure_decode_graph(p, slotn))) return rc;
    if (n_steps >= Plan::GRAPH_MULTI) {
        for (; s + Plan::GRAPH_MULTI <= n_steps; s += Plan::GRAPH_MULTI) if ((rc = p->graphs[slotn].launch(ctx))) return rc;
    }
    if (s < n_steps) {
        if ((rc = ensure_decode_graph(p, slot1))) return rc;
        for (; s < n_steps; ++s) if ((rc = p->graphs[slot1].launch(ctx))) return rc;
    }
    return 0;
}

static int upload_step_params(Plan* p, uint32_t slot, uint32_t token, uint32_t past, uint32_t step) {
    lh_ctx* ctx = p->ctx;
    LH_LAUNCH(k_set_step, dim3(1), dim3(1), 0, ctx->stream, p->sp_dev + slot, token, past, step);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

int plan_embeddings(Plan* p, uint32_t n, float** out) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (!m.last_stage() || n == 0 || n > p->n_cap) LH_FAIL(ctx, LH_EINVAL, "embeddings: the last Eval of this plan had no %u final rows", n);
    if (const int rc = grow(ctx, &p->emb, &p->emb_cap, n, (size_t)m.d * 4)) return rc;
    // every route of plan_eval leaves the residual rows behind the last layer in p->xa; RMSNorm (ml.go:1753-1812) then Mul by the norm weight
    // (ml.go:1877-1914): k_rmsnorm_rows' arithmetic (fp32 squares, f64 sum, one fp32 scale, two roundings per element)
    LH_LAUNCH(k_rmsnorm_rows, dim3(n), dim3(256), 0, ctx->stream, (const float*)p->xa, m.norm, p->emb, m.d);
    LH_HIP(ctx, hipGetLastError());
    *out = p->emb;
    return 0;
}

bool swap_refeed_tokens(const Plan* p, uint32_t past, uint32_t pending, std::vector<uint32_t>* out) {
    out->clear();
    if (p->keep > past) return false;
    const uint32_t n = (past - p->keep) / 2;
    if (n == 0) return true;
    for (uint32_t i = 0; i + 1 < n; ++i) {              // the n - 1 newest evaluated tokens ...
        const uint32_t idx = past - (n - 1) + i;
        const uint32_t t = (p->hist && idx < p->hist->size()) ? (*p->hist)[idx] : Plan::HIST_UNKNOWN;
        if (t == Plan::HIST_UNKNOWN) return false;
        out->push_back(t);
    }
    out->push_back(pending);                            // ... and the pending one, which lastNTokens already holds
    return true;
}

// n_steps resident decode steps (greedy: slots G_ADV*, sampled: G_SMP*) from the state in sp_dev[0] = {token, past, step}, with the reference's
// context swap whenever the window is full (server.go:160-172): the host then learns the ids produced so far (one synchronisation per
// (ctx - keep) / 2 tokens), re-feeds the run as ONE Eval at position keep and goes on.  first_token / past / step0 = what sp_dev[0] holds at
// entry; the ids produced by step i land in out_tokens_dev[step0 + i].  *past_io returns the position behind the last evaluated token.
// first_in_out (step0 >= 1): the first token is entry step0 - 1 of the output list (the sampler's pick behind the prompt) and is read together
// with the ids the steps produce - the caller need not synchronise for it up front (lh_llama_decode_sample paid a host round trip
// per generation for a value that is only needed at a swap or at the end).
static int resident_steps_swapping(Plan* p, uint32_t first_token, uint32_t* past_io, uint32_t step0, uint32_t n_steps, bool sampled, bool first_in_out = false) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& md = p->md;
    const int slot1 = sampled ? Plan::G_SMP1 : Plan::G_ADV1, slotn = sampled ? Plan::G_SMPN : Plan::G_ADVN;
    uint32_t past = *past_io, done = 0, pending = first_token;
    int rc;
    std::vector<uint32_t> got, refeed;
    // records the tokens evaluated by steps [from, done): step j evaluated (j == 0 ? first_token : the id step j - 1 produced) at position pos0 + (j - from)
    auto learn = [&](uint32_t from, uint32_t pos0) -> int {
        const uint32_t lead = (first_in_out && step0 >= 1) ? 1u : 0u;
        if (done == 0 && !lead) return 0;
        got.resize(done + 1);
        LH_HIP(ctx, hipMemcpyAsync(got.data() + 1 - lead, p->out_tokens_dev + step0 - lead, (size_t)(done + lead) * 4, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (lead) { first_token = got[0]; first_in_out = false; }   // (known from here on: later calls read the produced ids only)
        got.erase(got.begin());
        if (done == 0) { pending = first_token; return 0; }
        for (uint32_t j = from; j < done; ++j) p->record(pos0 + (j - from), j == 0 ? first_token : got[j - 1]);
        pending = got[done - 1];
        return 0;
    };
    uint32_t seg_from = 0, seg_pos0 = past;
    while (done < n_steps) {
        if (past >= md.ctx) {
            if ((rc = learn(seg_from, seg_pos0))) return rc;
            if (p->keep >= md.ctx) LH_FAIL(ctx, LH_EINVAL, "context swap: KeepCount %u leaves no room in a window of %u", p->keep, md.ctx);
            if (!swap_refeed_tokens(p, past, pending, &refeed))
                LH_FAIL(ctx, LH_EINVAL, "context swap at position %u: the tokens of the window are not known to this context (evaluate the prompt through it first)", past);
            if (!refeed.empty() && (rc = plan_eval(p, refeed.data(), nullptr, nullptr, (uint32_t)refeed.size(), p->keep, true))) return rc;
            past = p->keep + (uint32_t)refeed.size();
            if ((rc = upload_step_params(p, 0, pending, past, step0 + done))) return rc;
            seg_from = done; seg_pos0 = past;
        }
        const uint32_t k = std::min(n_steps - done, md.ctx - past);
        if (p->use_graph) {
            if ((rc = launch_resident_steps(p, k, slot1, slotn))) return rc;
        } else {
            for (uint32_t s2 = 0; s2 < k; ++s2)
                if ((rc = enqueue_decode(p, p->sp_dev, nullptr, nullptr, sampled ? 2 : 1, nullptr))) return rc;
        }
        done += k; past += k;
    }
    if ((rc = learn(seg_from, seg_pos0))) return rc;   // (also the synchronisation the callers' host copies wait for)
    *past_io = past;
    return 0;
}

int plan_decode_step(Plan* p, uint32_t token, uint32_t past) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (past >= m.ctx) LH_FAIL(ctx, LH_EINVAL, "decode: position %u outside the context window of %u", past, m.ctx);
    if (!m.first_stage() || !m.last_stage()) LH_FAIL(ctx, LH_EINVAL, "plan_decode_step needs a whole-model plan");
    p->record(past, token);
    int rc;
    if (p->use_graph) {
        if ((rc = ensure_decode_graph(p, Plan::G_STEP))) return rc;
        if ((rc = upload_step_params(p, 0, token, past, 0))) return rc;
        return p->graphs[Plan::G_STEP].launch(ctx);
    }
    if ((rc = upload_step_params(p, 0, token, past, 0))) return rc;
    return enqueue_decode(p, p->sp_dev, nullptr, nullptr, false, nullptr);
}

// ---- general Eval on the plan (N >= 1) ----------------------------------------------------------------
// block-int8 on k_stream_q8b: the shapes every launch of an Eval has an instantiation for (kernels_stream_q8b.h; <= 8 row tiles per workgroup
// in each of wq|wk|wv, w1|w3 pairs, the K-split fours of wo / w2 and the output matrix)
static bool q8b_shape_ok(lh_ctx* ctx, const ModelDesc& m) {
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, d = m.d, F = m.F;
    if (m.wtype != 7 || ncu < 4 || d > 8192 || d % 128 || F % 128 || m.hd % 4 || d % m.hd) return false;
    if ((3 * d / 16 + ncu - 1) / ncu > 8 || 2 * ((F / 16 + ncu - 1) / ncu) > 8 || (d / 16 + ncu / 4 - 1) / (ncu / 4) > 8) return false;
    if (m.last_stage() && (m.V % 16 || (m.V / 16 + ncu - 1) / ncu > 8)) return false;
    return true;
}
// fp32 weights on k_stream_b9 (round 6): the same layer schedule over planes, from four column tiles on (49..64 rows), where k_stream_dma's fp32-input
// MFMAs are the bound.  Inside the model (profiles/r06_pods64_kernel_trace_*.txt): w1|w3 112.7 -> 86.9 us, wo + w2 82 -> 73; at 33..48 rows the
// fp32 kernel is level or ahead (48 pods 6.99 against 7.08 ms per tick), and the standalone probe overstates ITS times by a quarter (random mantissas);
// every launch of the layer must have an instantiation (the output matrix may fall back to the fp32 rows the last reduce pass also writes).
static bool b9s_shape_ok(lh_ctx* ctx, const ModelDesc& m, uint32_t n) {
    const uint32_t ncu = (uint32_t)ctx->ds->num_cu, d = m.d, F = m.F;
    if (m.wtype != 0 || ncu < 4 || n < 2 || n > B9S_MAX_ROWS || d > 8192 || d % 128 || F % 128 || m.hd % 4 || d % m.hd) return false;
    auto split_maxt = [&](uint32_t K) {   // row tiles of a workgroup in gemm_q8b_split's launch of a d x K matrix
        const uint32_t ngrp = ncu / q8b_split_groups(K / (uint32_t)B9S_KC, ncu);
        return (d / 16 + ngrp - 1) / ngrp;
    };
    return stream_b9_built((3 * d / 16 + ncu - 1) / ncu, n) && stream_b9_built(2 * ((F / 16 + ncu - 1) / ncu), n) && stream_b9_built(split_maxt(d), n) && stream_b9_built(split_maxt(F), n);
}
static constexpr uint32_t Q8B_PROMPT_ROWS = 88;   // a prompt takes up to two 64-row passes; from 89 rows the tile GEMM k_gemm_q8b3 (one 128-row tile: 9.0-9.8 ms flat over
                                                  // 65..128 rows on 7B) is ahead of them (8.6 ms at 65 rows, 8.9 at 80, 9.75 at 96, 11.4 at 128: profiles/r05_gemm_q8b3_probe.txt)
static bool q8_stream_ok(lh_ctx* ctx, const ModelDesc& m, uint32_t n, uint32_t n_min, bool batch_rows = true) {
    return n >= n_min && n <= (batch_rows ? STREAM_ROWS_Q8 : Q8B_PROMPT_ROWS) && q8b_shape_ok(ctx, m);
}

// The layer schedules of an Eval.  eval_route picks one from the model's shapes, the row count and whether the rows belong to different streams;
// plan_eval runs it.
//   Step     one row: the decode step
//   Rows     2..8 rows (block-int8: 2..4) on the decode launches with NC activation rows each (kernels_rows.h)
//   Q8Steps  block-int8 without a k_stream_q8b launch, below the dequantising GEMM's rows or shapes: n single steps
//   Skinny   fp32, 2..8 rows of one stream where k_stream_* is not built for the shape: k_skinny
//   Planes   the activations as three bf16 planes: block-int8 on k_stream_q8b (3..64 rows of a batch, 3..88 of a prompt), fp32 at 49..64 rows on k_stream_b9
//   Prefill  everything else: the fp32 stream kernels and tile GEMMs, the dequantising GEMM, the column kernels
// f16 weights (wtype 1): Step and Rows on the f16 forms of their kernels (kernels_f16.h); for every other row count the route eval_route picks for a wtype-0
// model of the same shapes, run on that model's kernels over an fp32 image of the matrices (sched_md, route_layer below).
// Rows of different streams (BatchCtx) take ONE weight pass only on a route whose position-dependent kernels all read the row table: Rows and Planes,
// and Prefill with fp32 weights (k_stream_mm2's RoPE epilogue, k_rope_store, k_attention, k_attention_split).  Step, Q8Steps and Skinny do not read it, nor
// do Prefill's tile GEMM RoPE epilogue above 64 rows and its prompt attention kernels, which the at most BATCH_ROWS_MAX rows of a batch never take
// (plan_batch_rows_ok; lh_batch evaluates what it refuses row by row on the rows' own plans).
enum class EvalRoute { Step, Rows, Q8Steps, Skinny, Planes, Prefill };
static EvalRoute eval_route(lh_ctx* ctx, const ModelDesc& m, uint32_t n, bool batched) {
    if (n == 1) return EvalRoute::Step;
    if (rows_path_ok(ctx, m, n)) return EvalRoute::Rows;
    // block-int8: 5..64 rows of a tick / 5..88 of a prompt on k_stream_q8b (two 64-row passes from 65); from 89 rows the tile GEMM k_gemm_q8b3 (Prefill)
    const bool q8_stream = q8_stream_ok(ctx, m, n, 3, batched);
    if (m.wtype == 7 && !q8_stream && (n < Q8_GEMM_MIN_ROWS || m.d % GBK || m.F % GBK || m.hd % 32)) return EvalRoute::Q8Steps;
    if (!batched && skinny_ok(m, n) && !stream_shape_ok(ctx, m)) return EvalRoute::Skinny;   // k_skinny only where the streaming MFMA kernel is not built for the shape
    if (q8_stream) return EvalRoute::Planes;   // block-int8, up to 64 rows: the bf16 matrix pipe (kernels_stream_q8b.h)
    static const int b9s_min = getenv("LLAMAHIP_B9S_MIN") ? atoi(getenv("LLAMAHIP_B9S_MIN")) : (int)B9S_MIN_ROWS;   // (A/B switch of round 6's measurements: 65 = off)
    if (m.wtype == 0 && (int)n >= b9s_min && n <= B9S_MAX_ROWS) return EvalRoute::Planes;   // fp32, 49..64 rows: the same schedule over planes on k_stream_b9
    return EvalRoute::Prefill;
}
// Prefill's grouped MFMA launches: from 9 rows (tile GEMM), fp32 weights from 2 rows on the streaming MFMA kernel
static bool prefill_mfma(const ModelDesc& m, uint32_t n) { return (n >= MFMA_MIN_ROWS || (n >= 2 && m.wtype == 0)) && m.d % GBK == 0 && m.F % GBK == 0; }
static const ModelDesc& sched_md(const Plan* p);
bool plan_batch_rows_ok(const Plan* p, uint32_t n) {
    const ModelDesc& m = sched_md(p);
    if (n < 2 || n > BATCH_ROWS_MAX) return false;
    const EvalRoute route = eval_route(p->ctx, m, n, true);
    if (route == EvalRoute::Rows) return true;   // two to eight (block-int8: four) rows ride the decode stream itself
    // block-int8 on the stream kernel: from 3 rows (one pass of the dequantising stream kernel costs 4.9 ms on 7B whatever the row count <= 16, a single-row
    // int8 GEMV step 2.04 ms: two rows are faster one after the other - profiles/r03_pods_one_gpu.jsonl)
    if (m.wtype == 7) return route == EvalRoute::Planes;
    return (route == EvalRoute::Planes || route == EvalRoute::Prefill) && prefill_mfma(m, n);   // (fp32 Planes may hand the Eval to Prefill)
}

struct EvalCall {   // the arguments of one plan_eval
    const uint32_t* tokens_host;
    const float* x_in_dev;
    float* x_out_dev;
    uint32_t n, past;
    bool last_row_only;
    const BatchCtx* bc;
};
static float attn_scale(const ModelDesc& m) { return (float)(1.0 / sqrt((double)m.d / (double)m.H)); }
// What a route's schedule is chosen for and runs on: the plan's model - or, for an f16 model, its fp32 shadow (Plan::md_wide), so that eval_route picks
// what it picks for a wtype-0 model of the same shapes.  Step and Rows, which the same predicates admit for both, run on the model itself (sched_md is
// not asked there); Skinny, Planes and Prefill open with it and see an fp32 model.
// A block-int4 model (wtype 2) has a block-int8 shadow in the same way: Step, Rows and Q8Steps run on the nibbles, Planes and Prefill on the int8 image.
static const ModelDesc& sched_md(const Plan* p) { return p->md.wtype == 1 || p->md.wtype == 2 ? p->md_wide : p->md; }
// lh_ctx_set_f16_stream in the key of a captured graph whose launches may hold a stream launch (ticks, speculative passes): the switch and the count of its
// changes for an f16 plan, 0 for every other plan (the switch does nothing there).  f16_stream_sync, in front of CapturedGraph::run: a changed value also
// clears the warm bits - the kernels the new value chooses set their LDS attribute at their first launch (set_lds_once), which must be an eager one.
// A block-int4 plan carries lh_ctx_set_q4_stream in the same field in the same way (its k_stream_q8b launch sites then launch k_stream_q4b): one key field, the
// switch of the plan's own weight type - a plan has one weight type, so the two switches never meet in one key.
static uint64_t f16_stream_key(const Plan* p) {
    if (p->md.wtype == 1) return (p->ctx->f16_stream_gen << 1) | (uint64_t)p->ctx->f16_stream;
    if (p->md.wtype == 2) return (p->ctx->q4_stream_gen << 1) | (uint64_t)p->ctx->q4_stream;
    return 0;
}
template <typename G>
static void f16_stream_sync(G& graph, uint64_t* seen, uint64_t now) {
    if (*seen != now) { graph.warm = 0; *seen = now; }
}
// The matrices of layer il for a route that works on m (sched_md): the model's own, or the fp32 image after enqueuing its widening - one exact pass
// (k_widen_f16) per matrix in front of the layer's launches; the stream orders it behind the launches of the layer before, which read the same image.
static const LayerW& route_layer(Plan* p, const ModelDesc& m, uint32_t il) {
    if (&m != &p->md_wide) return m.layers[il];
    const LayerW& S = p->md.layers[il];
    const LayerW& W = m.layers[il];
    const uint64_t dd = (uint64_t)m.d * m.d, dF = (uint64_t)m.d * m.F;
    const float* src[7] = {S.wq, S.wk, S.wv, S.wo, S.w1, S.w3, S.w2};
    const float* dst[7] = {W.wq, W.wk, W.wv, W.wo, W.w1, W.w3, W.w2};
    for (int k = 0; k < 7; ++k) {   // (a launch error surfaces at the layer's hipGetLastError)
        if (p->md.wtype == 2) expand_q4_launch(p->ctx, src[k], (void*)dst[k], k < 4 ? dd : dF);
        else widen_f16_launch(p->ctx, src[k], (float*)dst[k], k < 4 ? dd : dF);
    }
    return W;
}
// the output matrix for a route's lm_head of more than one row (or over planes): as above
static const float* route_output(Plan* p, const ModelDesc& m) {
    if (&m == &p->md_wide) {
        if (p->md.wtype == 2) expand_q4_launch(p->ctx, p->md.output, p->wide_out, (uint64_t)m.V * m.d);
        else widen_f16_launch(p->ctx, p->md.output, p->wide_out, (uint64_t)m.V * m.d);
    }
    return m.output;
}
// The nibbles behind int8 image slots (a block-int4 plan with lh_ctx_set_q4_stream on: eval_planes, eval_prefill): w[g] of a launch names the image slot
// of a matrix whose n quants lie 4-bit at nib[g] and which is NOT expanded yet (HalfSrc's pattern).  expand: k_expand_q4 per matrix into its slot,
// directly in front of a launch that reads int8.
struct Q4Src {
    const float* nib[3];
    uint64_t n;
    void expand(lh_ctx* ctx, const float* const* w, uint32_t groups) const {
        for (uint32_t g = 0; g < groups; ++g) expand_q4_launch(ctx, nib[g], (void*)w[g], n);   // (a launch error surfaces at the layer's hipGetLastError)
    }
};
// One k_stream_q8b launch site over matrices that may still be nibbles: launch(w, wdt) is the site's gemm_q8b_group / gemm_q8b_split call.  The nibbles as
// they are where the 4-bit chain has the launch (every ST_NA of it is the int8 chain's, except the alignment of the nibble planes themselves); otherwise
// the int8 launch over the image, which is expanded only if that launch exists - asked with a prepare-only pass, which enqueues nothing - so that an
// expansion pass never stands in front of a launch that does not read it.
template <typename F>
static int q4_stream_src(lh_ctx* ctx, const Q4Src* qs, const float* const* w, uint32_t groups, F&& launch) {
    if (!qs) return launch(w, 7);
    int rs = launch(qs->nib, 2);
    if (rs != ST_NA) return rs;
    const bool was = g_prepare_only;
    g_prepare_only = true;
    rs = launch(w, 7);
    g_prepare_only = was;
    if (rs || was) return rs;
    qs->expand(ctx, w, groups);
    return launch(w, 7);
}
// the output matrix for ONE logits row on the decode stream: an f16 model's halves / a block-int4 model's nibbles as they are (k_gemv_sa_h / k_gemv_q4s
// compute the bits k_gemv_sa / k_gemv_q8s would over the image)
struct HeadRow { const float* w; int wtype; };
static HeadRow head_row(const Plan* p, const ModelDesc& m) { return &m == &p->md_wide ? HeadRow{p->md.output, p->md.wtype} : HeadRow{m.output, m.wtype}; }
// The logits rows of the last stage, first row and count: all n as the reference evaluates them (llama.go:372-384), or the last one alone, which is all
// llama.Eval reads (llama.go:394-401), for callers that say so (LH_GRAPH_LAST_ROW_LOGITS, the lh_llama_* entry points) - in its usual place.
struct LogitsRows { uint32_t r0, nr; };
static LogitsRows logits_rows(const EvalCall& c) { return c.last_row_only ? LogitsRows{c.n - 1, 1} : LogitsRows{0, c.n}; }

// The rows a route's first layer reads (*x): on the first stage the embeddings of the token ids in p->xa - a solo Eval's ids staged up from the host, a
// batch's already on the device - on a later stage the residual stream it received.  Rows keeps the launch out of a prepare-only pass; the prefill
// (and, behind the same launch, the planes) route names it for LLAMAHIP_TRACE.
static int eval_input(Plan* p, const EvalCall& c, EvalRoute route, const float** x) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (!m.first_stage()) { *x = c.x_in_dev; return 0; }
    *x = p->xa;
    const uint32_t* tok_dev = c.bc ? c.bc->tok_dev : p->tokens_dev;
    if (!c.bc) {
        if (const int rc = ensure_staging(ctx, (uint64_t)c.n * 4)) return rc;
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging reuse
        memcpy(ctx->staging, c.tokens_host, (size_t)c.n * 4);
        LH_HIP(ctx, hipMemcpyAsync(p->tokens_dev, ctx->staging, (size_t)c.n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    std::optional<TraceScope> ts_;
    if (route == EvalRoute::Planes || route == EvalRoute::Prefill) ts_.emplace(ctx->stream, "embedN");
    if (!(route == EvalRoute::Rows && g_prepare_only)) LH_LAUNCH(k_embed, dim3(c.n), dim3(256), 0, ctx->stream, m.tok_emb, tok_dev, (const StepParams*)nullptr, p->xa, m.d, m.V);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// The attention of a layer's n rows (llama.go:300-333) -> p->attn.  Rows of different streams: one query each, against its own cache up to its own
// position.  A prompt from 32 rows on, where the grouped MFMA launches run (mfma): one pass with an online softmax (head size 128), or batched MFMA GEMMs
// over heads with a score tensor (other head sizes).  Fewer queries: the per-query kernel (no score tensor) is cheaper.
// as != nullptr (Planes): the merged heads also as three bf16 planes of stride as_plane - the row-table and per-query kernels write them themselves, the
// prompt kernels' rows are split by a pass of their own.
static int eval_attention(Plan* p, const EvalCall& c, size_t slot, float scale, bool mfma, uint16_t* as = nullptr, uint64_t as_plane = 0) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    const uint32_t d = m.d, n = c.n, past = c.past;
    int rc;
    AttnArgs a = {};
    a.q = p->q; a.out = p->attn; a.d = d; a.hd = m.hd; a.n = n; a.scale = scale; a.out_s3 = as; a.out_plane = as_plane;
    if (c.bc) {
        a.rows = c.bc->rows; a.kv_off = slot;
        return launch_attention_rows(p, a, c.bc);
    }
    if (mfma && n >= 32 && (m.hd == FA_HD || m.hd % 32 == 0)) {
        if (m.hd == FA_HD) rc = attention_flash(p, p->q, m.kc + slot, m.vc + slot, p->attn, n, past, scale);
        else rc = attention_gemm(p, p->q, m.kc + slot, m.vc + slot, p->attn, n, past, scale);
        if (rc || !as) return rc;
        Split3Args sa = {p->attn, as, as_plane, d, d, d};
        if (!g_prepare_only) { TraceScope ts_(ctx->stream, "split3_rows"); LH_LAUNCH(k_split3_rows, dim3(n), dim3(256), 0, ctx->stream, sa); }
        return 0;
    }
    a.k_cache = m.kc + slot; a.v_cache = m.vc + slot; a.sp = nullptr; a.past_host = past;
    return launch_attention(ctx, a, past + n);
}

static int eval_step(Plan* p, const EvalCall& c) {
    const ModelDesc& m = p->md;
    if (m.first_stage() && m.last_stage() && p->use_graph) return plan_decode_step(p, c.tokens_host[0], c.past);
    const uint32_t slot = 1 + (p->slot_counter++ % (SP_SLOTS - 1));
    if (const int rc = upload_step_params(p, slot, c.tokens_host ? c.tokens_host[0] : 0, c.past, 0)) return rc;
    return enqueue_decode(p, p->sp_dev + slot, c.x_in_dev, c.x_out_dev, false, nullptr);
}

// 2..8 rows (block-int8: 2..4) (a prompt of that many tokens, or a tick of that many pods): the decode launches with NC activation rows each
// (kernels_rows.h): 5 launches per layer like the decode step, every row bit-identical to its solo step
static int eval_rows(Plan* p, const EvalCall& c, const float* x) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    const uint32_t n = c.n, past = c.past;
    const BatchRow* rows = c.bc ? c.bc->rows : nullptr;
    float* x_out_dev = c.x_out_dev;
    int rc;
    const float scale = attn_scale(m);
    const uint32_t d = m.d, F = m.F;
    for (uint32_t il = m.layer0; il < m.layer1; ++il) {
        const LayerW& L = m.layers[il];
        const size_t slot = (size_t)(il - m.cache_layer0) * m.ctx * d;
        {   // RMSNorm*gamma -> wq|wk|wv -> RoPE(Q, new K rows) -> K, V appended   (llama.go:255-297)
            GemvRowsArgs a = {};
            a.w[0] = L.wq; a.w[1] = L.wk; a.w[2] = L.wv; a.ws[0] = L.s_wq; a.ws[1] = L.s_wk; a.ws[2] = L.s_wv; a.rows_per_mat = d; a.M = 3 * d; a.K = d; a.x = x; a.ldx = d; a.n = n; a.gamma = L.attn_norm;
            a.q_out = p->q; a.k_cache = m.kc + slot; a.v_cache = m.vc + slot; a.rope = p->rope; a.hd = m.hd; a.d = d; a.past = past; a.rows = rows; a.kv_off = slot;
            if ((rc = gemv_rows<PRO_RMSNORM, EPI_QKV_ROPE, MAP_BLOCK>(ctx, a, "rows_qkv_rope", m.wtype))) return rc;
        }
        // scores, scale, mask, softmax, PV, head merge per row   (llama.go:300-333)
        if ((rc = eval_attention(p, c, slot, scale, false))) return rc;
        {   // wo + residual   (llama.go:336-340)
            GemvRowsArgs a = {};
            a.w[0] = L.wo; a.ws[0] = L.s_wo; a.M = d; a.K = d; a.x = p->attn; a.ldx = d; a.n = n; a.y = p->xb; a.resid = x; a.ldy = d;
            if ((rc = gemv_rows<PRO_PLAIN, EPI_RESID, MAP_SINGLE>(ctx, a, "rows_wo_resid", m.wtype))) return rc;
        }
        {   // RMSNorm*gamma -> w1|w3 -> silu(w1 h) * (w3 h)   (llama.go:346-361)
            GemvRowsArgs a = {};
            a.w[0] = L.w1; a.w[1] = L.w3; a.ws[0] = L.s_w1; a.ws[1] = L.s_w3; a.M = 2 * F; a.K = d; a.x = p->xb; a.ldx = d; a.n = n; a.gamma = L.ffn_norm; a.y = p->g; a.ldy = F;
            if ((rc = gemv_rows<PRO_RMSNORM, EPI_SILU_MUL, MAP_PAIR>(ctx, a, "rows_w1w3_silu", m.wtype))) return rc;
        }
        {   // w2 + residual   (llama.go:363-366)
            const bool last = il + 1 == m.layer1;
            GemvRowsArgs a = {};
            a.w[0] = L.w2; a.ws[0] = L.s_w2; a.M = d; a.K = F; a.x = p->g; a.ldx = F; a.n = n; a.resid = p->xb; a.ldy = d;
            a.y = (last && !m.last_stage()) ? x_out_dev : p->xa;
            if ((rc = gemv_rows<PRO_PLAIN, EPI_RESID, MAP_SINGLE>(ctx, a, "rows_w2_resid", m.wtype))) return rc;
        }
        x = p->xa;
    }
    if (m.last_stage()) {   // final RMSNorm*gamma -> lm_head: the rows the caller reads (llama.go:372-384, 394-401)
        const auto [r0, nr] = logits_rows(c);
        if (nr == 1) {
            GemvArgs a = {};
            a.w[0] = m.output; a.ws[0] = m.s_output; a.M = m.V; a.K = d; a.x = x + (size_t)r0 * d; a.gamma = m.norm; a.y = p->logits + (size_t)r0 * m.V;
            if ((rc = gemv<PRO_RMSNORM, EPI_STORE, MAP_SINGLE>(ctx, a, "gemv_lmhead", m.wtype))) return rc;
        } else {
            GemvRowsArgs a = {};
            a.w[0] = m.output; a.ws[0] = m.s_output; a.M = m.V; a.K = d; a.x = x + (size_t)r0 * d; a.ldx = d; a.n = nr; a.gamma = m.norm; a.y = p->logits + (size_t)r0 * m.V; a.ldy = m.V;
            if ((rc = gemv_rows<PRO_RMSNORM, EPI_STORE, MAP_SINGLE>(ctx, a, "rows_lmhead", m.wtype))) return rc;
        }
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// block-int8, short batches: n causal single-token steps on the int8 weight stream (bit-identical to what the decode
// path produces for them), logits row i from step i like llama.go:384.  n >= 32 takes the dequantising GEMM (Prefill).
// On a pipeline stage row i of the received / forwarded residual stream stands in for the token id / the logits row.
static int eval_q8_steps(Plan* p, const EvalCall& c) {
    const ModelDesc& m = p->md;
    const uint32_t n = c.n, past = c.past;
    const uint32_t* tokens_host = c.tokens_host;
    const float* x_in_dev = c.x_in_dev;
    float* x_out_dev = c.x_out_dev;
    int rc;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t slot = 1 + (p->slot_counter++ % (SP_SLOTS - 1));
        if ((rc = upload_step_params(p, slot, m.first_stage() ? tokens_host[i] : 0, past + i, 0))) return rc;
        if ((rc = enqueue_decode(p, p->sp_dev + slot, m.first_stage() ? nullptr : x_in_dev + (size_t)i * m.d, m.last_stage() ? nullptr : x_out_dev + (size_t)i * m.d, false,
                                 nullptr, nullptr, i)))
            return rc;
    }
    return 0;
}

// short prompt: 4 fused weight passes per layer + the per-query attention kernel (like the decode step, n rows wide)
static int eval_skinny(Plan* p, const EvalCall& c, const float* x) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = sched_md(p);
    const uint32_t n = c.n, past = c.past;
    float* x_out_dev = c.x_out_dev;
    int rc;
    const float scale = attn_scale(m);
    const uint32_t d = m.d, F = m.F;
    for (uint32_t il = m.layer0; il < m.layer1; ++il) {
        const LayerW& L = route_layer(p, m, il);
        const size_t slot = (size_t)(il - m.cache_layer0) * m.ctx * d;
        {   // RMSNorm*gamma -> wq|wk|wv -> RoPE(Q, new K rows) -> K,V appended   (llama.go:255-297)
            SkinnyArgs a = {};
            a.w[0] = L.wq; a.w[1] = L.wk; a.w[2] = L.wv; a.rows_per_mat = d; a.M = 3 * d; a.K = d; a.x = x; a.ldx = d; a.n = n; a.gamma = L.attn_norm;
            a.q_out = p->q; a.k_cache = m.kc + slot; a.v_cache = m.vc + slot; a.rope = p->rope; a.hd = m.hd; a.d = d; a.past = past;
            if ((rc = launch_skinny<PRO_RMSNORM, EPI_QKV_ROPE, MAP_BLOCK>(p, a, "skinny_qkv_rope"))) return rc;
        }
        if ((rc = eval_attention(p, c, slot, scale, false))) return rc;
        {   // wo + residual   (llama.go:336-340)
            SkinnyArgs a = {};
            a.w[0] = L.wo; a.M = d; a.K = d; a.x = p->attn; a.ldx = d; a.n = n; a.y = p->xb; a.resid = x; a.ldy = d;
            if ((rc = launch_skinny<PRO_PLAIN, EPI_RESID, MAP_SINGLE>(p, a, "skinny_wo_resid"))) return rc;
        }
        {   // RMSNorm*gamma -> w1|w3 -> silu(w1 h) * (w3 h)   (llama.go:346-361)
            SkinnyArgs a = {};
            a.w[0] = L.w1; a.w[1] = L.w3; a.M = 2 * F; a.K = d; a.x = p->xb; a.ldx = d; a.n = n; a.gamma = L.ffn_norm; a.y = p->g; a.ldy = F;
            if ((rc = launch_skinny<PRO_RMSNORM, EPI_SILU_MUL, MAP_PAIR>(p, a, "skinny_w1w3_silu"))) return rc;
        }
        {   // w2 + residual   (llama.go:363-366)
            const bool last = il + 1 == m.layer1;
            SkinnyArgs a = {};
            a.w[0] = L.w2; a.M = d; a.K = F; a.x = p->g; a.ldx = F; a.n = n; a.resid = p->xb; a.ldy = d;
            a.y = (last && !m.last_stage()) ? x_out_dev : p->xa;
            if ((rc = launch_skinny<PRO_PLAIN, EPI_RESID, MAP_SINGLE>(p, a, "skinny_w2_resid"))) return rc;
        }
        x = p->xa;
    }
    if (m.last_stage()) {   // final RMSNorm*gamma -> lm_head: the rows the caller reads (llama.go:372-384, 394-401)
        const auto [r0, nr] = logits_rows(c);
        if (nr == 1) {
            GemvArgs a = {};
            const HeadRow hw = head_row(p, m);
            a.w[0] = hw.w; a.M = m.V; a.K = d; a.x = x + (size_t)r0 * d; a.gamma = m.norm; a.y = p->logits + (size_t)r0 * m.V;
            if ((rc = gemv<PRO_RMSNORM, EPI_STORE, MAP_SINGLE>(ctx, a, "gemv_lmhead", hw.wtype))) return rc;
        } else {
            SkinnyArgs a = {};
            a.w[0] = route_output(p, m); a.M = m.V; a.K = d; a.x = x; a.ldx = d; a.n = n; a.gamma = m.norm; a.y = p->logits; a.ldy = m.V;
            if ((rc = launch_skinny<PRO_RMSNORM, EPI_STORE, MAP_SINGLE>(p, a, "skinny_lmhead"))) return rc;
        }
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// The layers over activation planes (three bf16 planes per activation matrix): block-int8 weights on k_stream_q8b, 3..64 rows of a tick or up to 88 of a
// prompt in two passes, and fp32 weights at 49..64 rows on k_stream_b9.  Per layer 7 launches:
//   [RMSNorm -> planes] (first layer only; afterwards the w2 reduce pass of the layer before writes them)
//   wq|wk|wv + RoPE + cache append | attention (merged heads -> planes) | wo as K-split fours | reduce + residual + RMSNorm -> planes |
//   w1|w3 + silu * mul -> planes | w2 as K-split fours | reduce + residual + the NEXT norm -> planes
// (llama.go:255-366).  Returns ST_NA before anything is enqueued when a launch of the model has no instantiation (plan_eval then
// hands an fp32 Eval to Prefill).
static int eval_planes(Plan* p, const EvalCall& c, const float* x) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = sched_md(p);
    const uint32_t n = c.n, past = c.past;
    const BatchRow* rows = c.bc ? c.bc->rows : nullptr;
    float* x_out_dev = c.x_out_dev;
    const uint32_t d = m.d, F = m.F;
    if (!(m.wtype == 7 ? q8b_shape_ok(ctx, m) : b9s_shape_ok(ctx, m, n))) return ST_NA;
    if (!p->s3 || n > p->s3_rows) return ST_NA;
    const float scale = attn_scale(m);
    const uint64_t pd = (uint64_t)p->s3_rows * d, pf = (uint64_t)p->s3_rows * F;   // plane strides (elements)
    uint16_t* hs = p->s3;
    uint16_t* as = hs + 3 * pd;
    uint16_t* gs = as + 3 * pd;
    int rc;
#define PLANES_TRY(expr, what) do { if ((rc = (expr))) { if (rc == ST_NA) LH_FAIL(ctx, LH_ESHAPE, "Eval of %u rows over activation planes: no launch for %s (embd %u, ff %u, weight type %u)", n, what, d, F, m.wtype); return rc; } } while (0)
    bool h_ready = false;
    // block-int4 plan with lh_ctx_set_q4_stream on: the launch sites read the model's own nibble planes (k_stream_q4b; the scale planes are the model's own
    // either way) and a matrix is expanded into its slot of the layer image only in front of a launch that reads int8 (Q4Src) - a layer whose launches
    // all stream enqueues no k_expand_q4.  m is the int8 shadow, so every decision here and down the chain is the expanded twin's.
    const bool q4s = &m == &p->md_wide && p->md.wtype == 2 && ctx->q4_stream;
    for (uint32_t il = m.layer0; il < m.layer1; ++il) {
        const LayerW& L = q4s ? m.layers[il] : route_layer(p, m, il);       // (q4s: the image slots, nothing in them yet)
        const LayerW& LS = q4s ? p->md.layers[il] : L;                       // the model's own matrices
        const uint64_t dd_ = (uint64_t)d * d, dF_ = (uint64_t)d * F;
        const Q4Src qqkv = {{LS.wq, LS.wk, LS.wv}, dd_}, qo = {{LS.wo}, dd_}, q13 = {{LS.w1, LS.w3}, dF_}, q2 = {{LS.w2}, dF_};
        auto src = [&](const Q4Src& q) -> const Q4Src* { return q4s ? &q : nullptr; };
        const size_t slot = (size_t)(il - m.cache_layer0) * m.ctx * d;
        if (!h_ready) { TraceScope ts_(ctx->stream, "rmsnorm_rows_s3"); if (!g_prepare_only) LH_LAUNCH(k_rmsnorm_rows_s3, dim3(n), dim3(256), 0, ctx->stream, x, L.attn_norm, (float*)nullptr, hs, pd, d); }
        {   // wq|wk|wv -> RoPE(Q, new K rows) -> K, V appended   (llama.go:263-297)
            const float* wqkv[3] = {L.wq, L.wk, L.wv};
            const float* sqkv[3] = {L.s_wq, L.s_wk, L.s_wv};
            StreamArgs fq = {};
            fq.epi = ST_EPI_QKV_ROPE; fq.q_out = p->q; fq.k_cache = m.kc + slot; fq.v_cache = m.vc + slot; fq.rope = p->rope; fq.hd = m.hd; fq.past = past;
            fq.rows = rows; fq.kv_off = slot;
            for (uint32_t b0 = 0; b0 < n; b0 += STREAM_ROWS_Q8) {   // (a prompt of 65..128 tokens: two passes over the weights, still 1.5x faster than the tile GEMM)
                const uint32_t nb = std::min(STREAM_ROWS_Q8, n - b0);
                fq.q_out = p->q + (size_t)b0 * d; fq.past = past + b0;
                PLANES_TRY(q4_stream_src(ctx, src(qqkv), wqkv, 3, [&](const float* const* ws, int wdt) {
                    return gemm_q8b_group(ctx, hs + (size_t)b0 * d, pd, d, 3, ws, sqkv, nullptr, nullptr, d, d, nb, d, m.wtype == 7 ? "q8b_wqkv_rope" : "b9s_wqkv_rope", &fq, wdt); }), "wq|wk|wv");
            }
        }
        if ((rc = eval_attention(p, c, slot, scale, true, as, pd))) return rc;   // merged heads -> planes (mfma: this route's shapes all have the grouped MFMA launches)
        // wo + residual + RMSNorm * ffn_norm -> planes   (llama.go:336-351)
        for (uint32_t b0 = 0; b0 < n; b0 += STREAM_ROWS_Q8)
            PLANES_TRY(q4_stream_src(ctx, src(qo), &L.wo, 1, [&](const float* const* ws, int wdt) {
                return gemm_q8b_split(ctx, ws[0], L.s_wo, as + (size_t)b0 * d, pd, d, d, d, std::min(STREAM_ROWS_Q8, n - b0), x + (size_t)b0 * d, p->xb + (size_t)b0 * d, L.ffn_norm, nullptr,
                                      hs + (size_t)b0 * d, pd, m.wtype == 7 ? "q8b_wo_ksplit" : "b9s_wo_ksplit", wdt); }), "wo");
        {   // w1|w3 -> silu(w1 h) * (w3 h) -> planes   (llama.go:354-361)
            const float* w13[2] = {L.w1, L.w3};
            const float* s13[2] = {L.s_w1, L.s_w3};
            StreamArgs fa = {};
            fa.epi = ST_EPI_SILU_MUL; fa.ys = gs; fa.ys_plane = pf; fa.ldys = F;
            for (uint32_t b0 = 0; b0 < n; b0 += STREAM_ROWS_Q8) {
                fa.ys = gs + (size_t)b0 * F;
                PLANES_TRY(q4_stream_src(ctx, src(q13), w13, 2, [&](const float* const* ws, int wdt) {
                    return gemm_q8b_group(ctx, hs + (size_t)b0 * d, pd, d, 2, ws, s13, nullptr, nullptr, F, d, std::min(STREAM_ROWS_Q8, n - b0), F, m.wtype == 7 ? "q8b_w1w3_silu" : "b9s_w1w3_silu", &fa, wdt); }), "w1|w3");
            }
        }
        {   // w2 + residual (+ the next layer's first norm, or the final norm, on the reduce pass)   (llama.go:363-372)
            const bool last = il + 1 == m.layer1;
            float* y = (last && !m.last_stage()) ? x_out_dev : p->xa;
            const float* next_gamma = !last ? m.layers[il + 1].attn_norm : (m.last_stage() ? m.norm : nullptr);
            for (uint32_t b0 = 0; b0 < n; b0 += STREAM_ROWS_Q8)
                PLANES_TRY(q4_stream_src(ctx, src(q2), &L.w2, 1, [&](const float* const* ws, int wdt) {
                    return gemm_q8b_split(ctx, ws[0], L.s_w2, gs + (size_t)b0 * F, pf, F, d, F, std::min(STREAM_ROWS_Q8, n - b0), p->xb + (size_t)b0 * d, y + (size_t)b0 * d, next_gamma,
                                          (last && m.last_stage()) ? p->h + (size_t)b0 * d : nullptr, next_gamma ? hs + (size_t)b0 * d : nullptr, pd, m.wtype == 7 ? "q8b_w2_ksplit" : "b9s_w2_ksplit", wdt); }), "w2");
            h_ready = next_gamma != nullptr;
        }
        x = p->xa;
        LH_HIP(ctx, hipGetLastError());
    }
    if (m.last_stage()) {   // lm_head on the rows the caller reads (llama.go:374-384, 394-401); hs / p->h hold RMSNorm * norm of every row
        const auto [r0, nr] = logits_rows(c);
        const float* wv = q4s ? m.output : route_output(p, m); const float* sv = m.s_output; float* yv = p->logits + (size_t)r0 * m.V;   // (m.output below: the same address)
        const Q4Src qout = {{p->md.output}, (uint64_t)m.V * d};
        const uint32_t hrow0 = r0;   // (a structured binding is not captured by a lambda before C++20)
        for (uint32_t b0 = 0; b0 < nr; b0 += STREAM_ROWS_Q8) {
            float* yb = yv + (size_t)b0 * m.V;
            const uint32_t nb = std::min(STREAM_ROWS_Q8, nr - b0);
            rc = q4_stream_src(ctx, q4s ? &qout : nullptr, &wv, 1, [&](const float* const* ws, int wdt) {
                return gemm_q8b_group(ctx, hs + (size_t)(hrow0 + b0) * d, pd, d, 1, ws, &sv, &yb, nullptr, m.V, d, nb, m.V, m.wtype == 7 ? "q8b_lmhead" : "b9s_lmhead", nullptr, wdt); });
            if (rc == ST_NA && m.wtype == 0 && nb > 1 && m.V % 32 == 0) {
                // fp32 output matrix with eight row tiles per workgroup next to four column tiles (7B at 49..64 rows): no k_stream_b9 launch of that shape - the two halves
                // of the vocabulary have one each (four row tiles).  64 pods, 7B: 172 us on k_stream_dma -> see profiles/r06_lmhead_halves.txt
                const uint32_t Vh = m.V / 2;
                const float* wh[2] = {m.output, m.output + (size_t)Vh * d};
                float* yh[2] = {yb, yb + Vh};
                for (int h2 = 0; h2 < 2; ++h2)
                    if ((rc = gemm_q8b_group(ctx, hs + (size_t)(r0 + b0) * d, pd, d, 1, &wh[h2], &sv, &yh[h2], nullptr, Vh, d, nb, m.V, "b9s_lmhead"))) break;
            }
            if (rc == ST_NA && m.wtype == 0) {   // fp32 output matrix without a k_stream_b9 launch (eight row tiles next to four column tiles): the fp32 rows
                if (nb == 1) {
                    GemvArgs ga = {};
                    ga.w[0] = m.output; ga.M = m.V; ga.K = d; ga.x = p->h + (size_t)(r0 + b0) * d; ga.y = yb;
                    rc = gemv<PRO_PLAIN, EPI_STORE, MAP_SINGLE>(ctx, ga, "gemv_lmhead_row", 0);
                } else rc = gemm_small_n(ctx, m.output, p->h + (size_t)(r0 + b0) * d, yb, nullptr, m.V, d, nb, d, m.V, "gemm_lmhead");
            }
            PLANES_TRY(rc, "lm_head");
        }
    }
    LH_HIP(ctx, hipGetLastError());
#undef PLANES_TRY
    return 0;
}

// prefill, N > 1 rows (or the rows of a batched Eval: `rows` set, every row at its own position of its own cache): the fp32 stream kernels and tile GEMMs,
// the dequantising GEMM of block-int8 weights, the column kernels for what neither takes
static int eval_prefill(Plan* p, const EvalCall& c, const float* x) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = sched_md(p);
    const uint32_t n = c.n, past = c.past, d = m.d, F = m.F;
    const BatchCtx* bc = c.bc;
    const BatchRow* rows = bc ? bc->rows : nullptr;
    float* x_out_dev = c.x_out_dev;
    const double2* rope = p->rope;
    const float scale = attn_scale(m);
    int rc;
    // fp32 prompts just past the stream kernels' 128 rows: two passes over the weights, ceil(n / 2) rows each (the rows of a pass are independent of the other
    // pass's in every launch but attention, which runs once over all n as before).  Measurements: STREAM_TWO_PASS_MAX.
    static const uint32_t two_pass_max = getenv("LLAMAHIP_TWO_PASS_MAX") ? (uint32_t)atoi(getenv("LLAMAHIP_TWO_PASS_MAX")) : STREAM_TWO_PASS_MAX;   // (A/B switch: 128 = off)
    const bool two_pass = !bc && m.wtype == 0 && n > stream_max_rows() && n <= two_pass_max && n <= 2 * stream_max_rows() && d % GBK == 0 && F % GBK == 0 && stream_shape_ok(ctx, m);
    const uint32_t sb = two_pass ? (n + 1) / 2 : n;   // rows per pass of the stream kernels
    bool h_ready = false;   // p->h already holds this layer's RMSNorm * attn_norm rows (written by the previous layer's w2 reduce pass)
    // f16 plan with lh_ctx_set_f16_stream on: the stream launch sites read the model's own halves (k_stream_mm2_h / k_stream_dma_h), and a matrix is
    // widened into its slot of the layer image only when a launch that reads fp32 is about to read it (HalfSrc) - a layer whose launches all stream
    // enqueues no k_widen_f16.  m is then the fp32 shadow, so every decision below is the widened twin's.
    // lh_ctx_set_f16_tiles: the same hand-out for the tile GEMM - a k_gemm_b9 launch reads the halves (k_gemm_b9_h, kernels_gemm_f16.h).  Either switch
    // makes the matrices lazy; which launches read halves is each switch's own (HalfSrc::stream / ::tiles).
    const bool f16p = &m == &p->md_wide && p->md.wtype == 1;
    const bool hstream = f16p && ctx->f16_stream, htiles = f16p && ctx->f16_tiles, lazy = hstream || htiles;
    // block-int4 plan with lh_ctx_set_q4_stream on: no launch of this route reads nibbles (k_gemm_q8b3 and the dequantising GEMM read int8), so every matrix
    // is expanded - directly in front of the launch that reads it (q4x below) instead of in front of the layer, the one place an expansion stands under
    // the switch (eval_planes, Q4Src).  A plan whose shapes have no k_stream_q8b schedule never launches k_stream_q4b: the switch leaves it alone entirely.
    const bool q4s = &m == &p->md_wide && p->md.wtype == 2 && ctx->q4_stream && q8b_shape_ok(ctx, m);
    for (uint32_t il = m.layer0; il < m.layer1; ++il) {
        const LayerW& L = (lazy || q4s) ? m.layers[il] : route_layer(p, m, il);   // (lazy, q4s: the image slots, nothing in them yet)
        const LayerW& LS = (lazy || q4s) ? p->md.layers[il] : L;                  // the model's own matrices
        const Q4Src qqkv = {{LS.wq, LS.wk, LS.wv}, (uint64_t)d * d}, qo = {{LS.wo}, (uint64_t)d * d}, q13 = {{LS.w1, LS.w3}, (uint64_t)d * F}, q2 = {{LS.w2}, (uint64_t)d * F};
        auto q4x = [&](const Q4Src& q, const float* const* w, uint32_t groups) { if (q4s) q.expand(ctx, w, groups); };
        bool wide[7] = {};                                                  // wq wk wv wo w1 w3 w2: the slot holds the matrix
        const uint64_t dd_ = (uint64_t)d * d, dF_ = (uint64_t)d * F;
        const HalfSrc hqkv = {{LS.wq, LS.wk, LS.wv}, dd_, {&wide[0], &wide[1], &wide[2]}, hstream, htiles}, hq = {{LS.wq}, dd_, {&wide[0]}, hstream, htiles},
                      hk = {{LS.wk}, dd_, {&wide[1]}, hstream, htiles}, hv = {{LS.wv}, dd_, {&wide[2]}, hstream, htiles}, ho = {{LS.wo}, dd_, {&wide[3]}, hstream, htiles},
                      h13 = {{LS.w1, LS.w3}, dF_, {&wide[4], &wide[5]}, hstream, htiles}, h1 = {{LS.w1}, dF_, {&wide[4]}, hstream, htiles},
                      h3 = {{LS.w3}, dF_, {&wide[5]}, hstream, htiles}, h2 = {{LS.w2}, dF_, {&wide[6]}, hstream, htiles};
        auto src = [&](const HalfSrc& h) -> const HalfSrc* { return lazy ? &h : nullptr; };
        const size_t slot = (size_t)(il - m.cache_layer0) * m.ctx * d;
        const bool mfma = prefill_mfma(m, n);
        const bool q8 = m.wtype == 7;
        bool qkv_roped = false, gated = false;
        // 17..64 rows: wo / w2 as K-split pairs whose reduce pass also writes the next norm's rows into p->h (gemm_stream_split)
        const bool ksp = sb > 16 && sb <= stream_max_rows() && !q8 && mfma;
        bool hf_ready = false;
        const float* wqkv[3] = {L.wq, L.wk, L.wv};
        const float* sqkv[3] = {L.s_wq, L.s_wk, L.s_wv};
        float* yqkv[3] = {p->qraw, p->kraw, p->vraw};
        // RoPE + cache append in the GEMM's epilogue (no rope_store pass, no raw q/k/v round trip): where each row goes
        StreamArgs fq = {};
        fq.epi = ST_EPI_QKV_ROPE; fq.q_out = p->q; fq.k_cache = m.kc + slot; fq.v_cache = m.vc + slot; fq.rope = rope; fq.hd = m.hd; fq.past = past;
        fq.rows = rows; fq.kv_off = slot;
        const bool fold_norm = n <= 16 && !q8 && mfma;
        if (n <= stream_max_rows() && fold_norm) {
            // short prompts: ONE launch for RMSNorm (folded: gamma at staging, the per-token scale in the epilogue) -> wq|wk|wv -> RoPE -> cache append
            // (folded up to 16 rows: -3..5 % per Eval; at 17..32 rows the extra staging work of the loader waves eats the saved launch)
            StreamArgs fa = fq;
            fa.gamma = L.attn_norm;
            const int rs = stream_src(ctx, src(hqkv), wqkv, 3, [&](const float* const* ws, int wdt) { return gemm_stream_group(ctx, x, d, 3, ws, nullptr, nullptr, d, d, n, d, "stream_norm_wqkv_rope", &fa, wdt); });
            if (rs < 0) return rs;
            qkv_roped = rs == 0;
        }
        if (!qkv_roped && !h_ready) { TraceScope ts_(ctx->stream, "rmsnorm_rows_a"); LH_LAUNCH(k_rmsnorm_rows, dim3(n), dim3(256), 0, ctx->stream, x, L.attn_norm, p->h, d); }
        h_ready = false;
        if (qkv_roped) {
        } else if (q8) {   // (prompts beyond k_stream_q8b's 64 rows)
            q4x(qqkv, wqkv, 3);
            if ((rc = gemm_q8_group(ctx, p->h, d, 3, wqkv, sqkv, yqkv, nullptr, d, d, n, d, "gemm_q8_wqkv"))) return rc;
        } else if (mfma) {
            int rs = ST_NA;
            for (uint32_t b0 = 0; b0 < n && sb <= stream_max_rows(); b0 += sb) {
                StreamArgs fb = fq;
                fb.q_out = p->q + (size_t)b0 * d; fb.past = past + b0;
                if ((rs = stream_src(ctx, src(hqkv), wqkv, 3, [&](const float* const* ws, int wdt) { return gemm_stream_group(ctx, p->h + (size_t)b0 * d, d, 3, ws, nullptr, nullptr, d, d, std::min(sb, n - b0), d, "stream_wqkv_rope", &fb, wdt); }))) break;
            }
            if (rs == ST_NA && n > 64) {   // long prompts: the same epilogue in the tile GEMM
                GemmArgs ga = {};
                ga.epi = GEMM_EPI_QKV_ROPE; ga.q_out = p->q; ga.k_cache = m.kc + slot; ga.v_cache = m.vc + slot; ga.rope = rope; ga.hd = m.hd; ga.past = past;
                rs = gemm_mfma_group(ctx, p->h, d, 3, wqkv, nullptr, nullptr, d, d, n, d, "gemm_wqkv_rope", &ga, true, src(hqkv));
            }
            if (rs < 0) return rs;
            qkv_roped = rs == 0;
            if (!qkv_roped && (rc = gemm_mfma_group(ctx, p->h, d, 3, wqkv, yqkv, nullptr, d, d, n, d, "gemm_wqkv", nullptr, true, src(hqkv)))) return rc;
        } else {
            if ((rc = gemm_small_n_src(ctx, L.wq, p->h, p->qraw, nullptr, d, d, n, d, d, "gemm_wq", true, src(hq)))) return rc;
            if ((rc = gemm_small_n_src(ctx, L.wk, p->h, p->kraw, nullptr, d, d, n, d, d, "gemm_wk", true, src(hk)))) return rc;
            if ((rc = gemm_small_n_src(ctx, L.wv, p->h, p->vraw, nullptr, d, d, n, d, d, "gemm_wv", true, src(hv)))) return rc;
        }
        if (!qkv_roped) { TraceScope ts_(ctx->stream, "rope_store"); LH_LAUNCH(k_rope_store, dim3(n), dim3(256), 0, ctx->stream, (const float*)p->qraw, (const float*)p->kraw, (const float*)p->vraw, p->q, m.kc + slot,
                           m.vc + slot, rope, d, m.hd, past, rows, (uint64_t)slot); }
        if ((rc = eval_attention(p, c, slot, scale, mfma))) return rc;
        int wo_rs = ST_NA;
        if (ksp) {
            for (uint32_t b0 = 0; b0 < n; b0 += sb)
                if ((wo_rs = stream_src(ctx, src(ho), &L.wo, 1, [&](const float* const* ws, int wdt) { return gemm_stream_split(ctx, ws[0], p->attn + (size_t)b0 * d, d, d, d, std::min(sb, n - b0), x + (size_t)b0 * d, p->xb + (size_t)b0 * d, L.ffn_norm, p->h + (size_t)b0 * d, "stream_wo_ksplit", wdt); }))) break;
            if (wo_rs < 0) return wo_rs;
            hf_ready = wo_rs == 0;
        }
        if (wo_rs == 0) {
        } else if (q8) { q4x(qo, &L.wo, 1); if ((rc = gemm_q8(ctx, L.wo, L.s_wo, p->attn, p->xb, x, d, d, n, d, d, "gemm_q8_wo"))) return rc; }
        else if ((rc = gemm_small_n_src(ctx, L.wo, p->attn, p->xb, x, d, d, n, d, d, "gemm_wo", true, src(ho)))) return rc;
        const float* w13[2] = {L.w1, L.w3};
        const float* s13[2] = {L.s_w1, L.s_w3};
        float* y13[2] = {p->a1, p->a3};
        float* yg[2] = {p->g, nullptr};
        if (n <= stream_max_rows() && fold_norm) {   // short prompts: RMSNorm (folded) -> w1|w3 -> silu * mul in one launch
            StreamArgs fa = {};
            fa.epi = ST_EPI_SILU_MUL;
            fa.gamma = L.ffn_norm;
            const int rs = stream_src(ctx, src(h13), w13, 2, [&](const float* const* ws, int wdt) { return gemm_stream_group(ctx, p->xb, d, 2, ws, yg, nullptr, F, d, n, F, "stream_norm_w1w3_silu", &fa, wdt); });
            if (rs < 0) return rs;
            gated = rs == 0;
        }
        if (!gated && !hf_ready) { TraceScope ts_(ctx->stream, "rmsnorm_rows_f"); LH_LAUNCH(k_rmsnorm_rows, dim3(n), dim3(256), 0, ctx->stream, (const float*)p->xb, L.ffn_norm, p->h, d); }
        if (gated) {
        } else if (q8) {
            q4x(q13, w13, 2);
            if ((rc = gemm_q8_group(ctx, p->h, d, 2, w13, s13, y13, nullptr, F, d, n, F, "gemm_q8_w1w3"))) return rc;
        } else if (mfma) {
            StreamArgs fa = {};   // short prompts: silu(w1 h) * (w3 h) in the epilogue of (w1, w3) tile pairs
            fa.epi = ST_EPI_SILU_MUL;
            int rs = ST_NA;
            for (uint32_t b0 = 0; b0 < n && sb <= stream_max_rows(); b0 += sb) {
                float* ygb[2] = {p->g + (size_t)b0 * F, nullptr};
                if ((rs = stream_src(ctx, src(h13), w13, 2, [&](const float* const* ws, int wdt) { return gemm_stream_group(ctx, p->h + (size_t)b0 * d, d, 2, ws, ygb, nullptr, F, d, std::min(sb, n - b0), F, "stream_w1w3_silu", &fa, wdt); }))) break;
            }
            if (rs == ST_NA && n > 64) {
                GemmArgs ga = {};
                ga.epi = GEMM_EPI_SILU_MUL;
                rs = gemm_mfma_group(ctx, p->h, d, 2, w13, yg, nullptr, F, d, n, F, "gemm_w1w3_silu", &ga, true, src(h13));
            }
            if (rs < 0) return rs;
            gated = rs == 0;
            if (!gated && (rc = gemm_mfma_group(ctx, p->h, d, 2, w13, y13, nullptr, F, d, n, F, "gemm_w1w3", nullptr, true, src(h13)))) return rc;
        } else {
            if ((rc = gemm_small_n_src(ctx, L.w1, p->h, p->a1, nullptr, F, d, n, d, F, "gemm_w1", true, src(h1)))) return rc;
            if ((rc = gemm_small_n_src(ctx, L.w3, p->h, p->a3, nullptr, F, d, n, d, F, "gemm_w3", true, src(h3)))) return rc;
        }
        if (!gated) { TraceScope ts_(ctx->stream, "silu_mul"); LH_LAUNCH(k_silu_mul, dim3(std::min<uint64_t>(((uint64_t)n * F + 255) / 256, 4096)), dim3(256), 0, ctx->stream, (const float*)p->a1,
                           (const float*)p->a3, p->g, (uint64_t)n * F); }
        const bool last = il + 1 == m.layer1;
        float* y = (last && !m.last_stage()) ? x_out_dev : p->xa;
        int w2_rs = ST_NA;
        if (ksp) {
            const float* next_gamma = last ? nullptr : m.layers[il + 1].attn_norm;   // the next layer's first norm rides on the reduce pass
            for (uint32_t b0 = 0; b0 < n; b0 += sb)
                if ((w2_rs = stream_src(ctx, src(h2), &L.w2, 1, [&](const float* const* ws, int wdt) { return gemm_stream_split(ctx, ws[0], p->g + (size_t)b0 * F, F, d, F, std::min(sb, n - b0), p->xb + (size_t)b0 * d, y + (size_t)b0 * d, next_gamma, p->h + (size_t)b0 * d, "stream_w2_ksplit", wdt); }))) break;
            if (w2_rs < 0) return w2_rs;
            h_ready = w2_rs == 0 && next_gamma != nullptr;
        }
        if (w2_rs == 0) {
        } else if (q8) { q4x(q2, &L.w2, 1); if ((rc = gemm_q8(ctx, L.w2, L.s_w2, p->g, y, p->xb, d, F, n, F, d, "gemm_q8_w2"))) return rc; }
        else if ((rc = gemm_small_n_src(ctx, L.w2, p->g, y, p->xb, d, F, n, F, d, "gemm_w2", true, src(h2)))) return rc;
        x = p->xa;
        LH_HIP(ctx, hipGetLastError());
    }
    if (m.last_stage()) {
        // the reference evaluates norm + lm_head for all N rows (llama.go:372-384) although only row N-1 is read (llama.go:394-401);
        // callers that say so (LH_GRAPH_LAST_ROW_LOGITS, the lh_llama_* entry points) get that row only, in its usual place
        const auto [r0, nr] = logits_rows(c);
        { TraceScope ts_(ctx->stream, "rmsnorm_rows_final"); LH_LAUNCH(k_rmsnorm_rows, dim3(nr), dim3(256), 0, ctx->stream, x + (size_t)r0 * d, m.norm, p->h + (size_t)r0 * d, d); }
        if (m.wtype == 7) {
            if (nr >= Q8_GEMM_MIN_ROWS) {
                if ((rc = gemm_q8(ctx, route_output(p, m), m.s_output, p->h + (size_t)r0 * d, p->logits + (size_t)r0 * m.V, nullptr, m.V, d, nr, d, m.V, "gemm_q8_lmhead"))) return rc;
            } else {   // a few rows (the last row of a long prompt): the int8 GEMV row by row (one row of a block-int4 model: on its nibbles)
                const HeadRow hw = nr == 1 ? head_row(p, m) : HeadRow{route_output(p, m), 7};
                for (uint32_t i = 0; i < nr; ++i) {
                    GemvArgs ga = {};
                    ga.w[0] = hw.w; ga.ws[0] = m.s_output; ga.M = m.V; ga.K = d; ga.x = p->h + (size_t)(r0 + i) * d; ga.y = p->logits + (size_t)(r0 + i) * m.V;
                    if ((rc = gemv<PRO_PLAIN, EPI_STORE, MAP_SINGLE>(ctx, ga, "gemv_lmhead_row", hw.wtype))) return rc;
                }
            }
        } else if (nr == 1) {   // the one row llama.Eval reads: the decode weight stream (76 us on 7B; the column kernel took 122)
            GemvArgs ga = {};
            const HeadRow hw = head_row(p, m);
            ga.w[0] = hw.w; ga.M = m.V; ga.K = d; ga.x = p->h + (size_t)r0 * d; ga.y = p->logits + (size_t)r0 * m.V;
            if ((rc = gemv<PRO_PLAIN, EPI_STORE, MAP_SINGLE>(ctx, ga, "gemv_lmhead_row", hw.wtype))) return rc;
        } else if (htiles) {   // the output matrix lazily: halves where the twin's launch is k_gemm_b9, one widening pass directly in front of any other launch
            bool wide_out = false;
            const HalfSrc hout = {{p->md.output}, (uint64_t)m.V * d, {&wide_out}, false, true};
            if ((rc = gemm_small_n_src(ctx, m.output, p->h + (size_t)r0 * d, p->logits + (size_t)r0 * m.V, nullptr, m.V, d, nr, d, m.V, "gemm_lmhead", true, &hout))) return rc;
        } else if ((rc = gemm_small_n(ctx, route_output(p, m), p->h + (size_t)r0 * d, p->logits + (size_t)r0 * m.V, nullptr, m.V, d, nr, d, m.V, "gemm_lmhead"))) return rc;
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

int plan_eval(Plan* p, const uint32_t* tokens_host, const float* x_in_dev, float* x_out_dev, uint32_t n, uint32_t past, bool last_row_only, const BatchCtx* bc) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (n == 0) LH_FAIL(ctx, LH_EINVAL, "Eval: empty token batch");
    if (bc) {
        if (!bc->rows || (m.first_stage() && !bc->tok_dev) || !plan_batch_rows_ok(p, n)) LH_FAIL(ctx, LH_EINVAL, "Eval: batched rows need a row table, token ids and a supported shape");
        if (n > p->n_cap) LH_FAIL(ctx, LH_EINVAL, "Eval: batched rows exceed the plan's scratch (plan_ensure_rows first: a captured graph must not allocate)");
    } else {
        if ((uint64_t)past + n > m.ctx) LH_FAIL(ctx, LH_EINVAL, "Eval: past %u + n %u exceeds the context window of %u", past, n, m.ctx);
        if (m.first_stage() && !tokens_host) LH_FAIL(ctx, LH_EINVAL, "Eval: first stage needs token ids");
        if (m.first_stage())  // Go panics on tokEmbeddings.Data[id*NE[0]:] past the table (ml.go:1748); the GPU must never gather out of range
            for (uint32_t i = 0; i < n; ++i)
                if (tokens_host[i] >= m.V) LH_FAIL(ctx, LH_EINVAL, "Eval: token id %u at index %u outside the vocabulary of %u", tokens_host[i], i, m.V);
        if (m.first_stage()) for (uint32_t i = 0; i < n; ++i) p->record(past + i, tokens_host[i]);
        if (past < p->share_len) p->share_broken = true;   // this Eval writes cache rows of a shared prefix: the pod's batch drops it from its group (lh_batch_fork)
    }
    if (!m.first_stage() && !x_in_dev) LH_FAIL(ctx, LH_EINVAL, "Eval: later stage needs the residual stream");
    if (!m.last_stage() && !x_out_dev) LH_FAIL(ctx, LH_EINVAL, "Eval: non-final stage needs an output buffer");
    int rc;
    if (!bc && (rc = plan_ensure_rows(p, n))) return rc;
    const EvalCall c = {tokens_host, x_in_dev, x_out_dev, n, past, last_row_only, bc};
    const EvalRoute route = eval_route(ctx, sched_md(p), n, bc != nullptr);
    const float* x = nullptr;   // the rows the first layer reads
    if (route != EvalRoute::Step && route != EvalRoute::Q8Steps && (rc = eval_input(p, c, route, &x))) return rc;   // (the single steps embed their own token)
    switch (route) {
        case EvalRoute::Step: return eval_step(p, c);
        case EvalRoute::Rows: return eval_rows(p, c, x);
        case EvalRoute::Q8Steps: return eval_q8_steps(p, c);
        case EvalRoute::Skinny: return eval_skinny(p, c, x);
        case EvalRoute::Planes:
            rc = eval_planes(p, c, x);
            if (rc != ST_NA) return rc;
            if (sched_md(p).wtype == 7) LH_FAIL(ctx, LH_ESHAPE, "block-int8 Eval of %u rows: the plan's shape has no k_stream_q8b launch", n);
            break;   // fp32: ST_NA comes back before anything but the embedding is enqueued, and the fp32-MFMA route takes the Eval
        case EvalRoute::Prefill: break;
    }
    return eval_prefill(p, c, x);
}


// ---- lh_batch: the pods of a rank in ONE weight pass ---------------------------------------------------------------------------
// The reference's only parallelism is request-level: Engine() runs up to MaxPods Do() goroutines (pkg/server/server.go:84-106), each with
// its own llama.Context over the shared Model (server.go:151).  On the GPU an N = 1 Eval streams all weights, so P pods that decode
// independently read P x 26.4 GB per round of tokens for the bandwidth of one.  A batch binds the stages of P streams (same weights and
// layer range, one KV cache each) and evaluates one decode step of ALL of them as a P-row pass: the stream GEMMs of the short-prompt path
// (k_stream_mm2: every weight byte read once for all rows), RoPE / cache append / attention per row from a device table
// {row -> its cache, its position}.  Row results do not depend on the row's index or on the other rows (every output column of the MFMA
// tiles accumulates on its own), so a stream decodes the same ids whoever shares its tick.
// One tick = one captured hipGraph (token ids, positions and the residual stream live at fixed device addresses; the graph itself moves the
// positions on), so a tick costs the host one hipGraphLaunch whatever the stage's length.
struct BatchSpec;
struct Batch {
    lh_ctx* ctx = nullptr;
    std::vector<Plan*> pods;
    uint32_t B = 0;
    bool batched = false;          // rows share one weight pass (else: row by row on their own plans - same results, P weight passes)
    BatchRow* rows_dev = nullptr;  // [B]
    uint32_t* tok_dev = nullptr;   // [B] token ids of the next tick (first stage)
    uint32_t* ids_dev = nullptr;   // [B] ids produced by the last tick (last stage)
    uint32_t* out_dev = nullptr;   // [B][out_cap] ids produced per row (last stage)
    uint32_t out_cap = 0;
    StepParams* sp_dev = nullptr;  // [B] the rows' step parameters, in lockstep with rows_dev (what the N = 1 kernels and the sampler read)
    float* logits_own = nullptr;   // [B][V] row-by-row mode with B > 1 (last stage)
    float* attn_part = nullptr;    // batched, ctx > 256: split-T attention partials for B rows
    // sampling ticks (lh_batch_set_sampler): per-row sampler state + lastNTokens ring
    SampleState* ss_dev = nullptr; // [B]
    uint32_t* ring_dev = nullptr;  // [B][ring_cap]
    uint32_t ring_cap = 0, smp_topk = 0;
    uint32_t ring_size = 0;        // of the last lh_batch_set_sampler (lh_batch_sampler_ring_size)
    bool sampling = false;
    uint64_t smp_gen = 0;          // counts what the captured tick holds and lh_batch_set_sampler changes: the ring's address, the kernel variant (topK <= 64 or not)
    // the captured tick (warm bit 0) and everything it holds by value
    struct TickKey {
        const float* x_in;
        float* x_out;
        uint64_t splitk_gen, scratch_gen, smp_gen;
        uint32_t sampling, per_pod, shared, share_qb;   // (share_qb: 0 unless shared)
        uint64_t f16_stream;                            // f16_stream_key: 0 unless the pods are f16 plans
    };
    CapturedGraph<TickKey> tick;
    uint64_t f16_seen = 0;         // f16_stream_sync: the key value the tick / the speculative pass last ran with
    uint64_t scratch_gen() const { uint64_t g = 0; for (const Plan* p : pods) g += p->scratch_gen; return g; }   // grows when any pod's scratch moved
    bool per_pod = false;          // LLAMAHIP_SAMPLE_PER_POD=1: one sampler launch per row (read where the tick is enqueued)
    // host mirror of the rows' positions (rows_dev[i].pos): the tick kernels advance them in device memory with no bound of their own, so
    // the window check of every other Eval entry point (plan_eval: past + n <= ctx) is made here before a tick is enqueued
    std::vector<uint32_t> pos;
    bool pos_known = false;        // false until lh_batch_set / lh_batch_prompt placed the rows
    // Context swap (server.go:160-172) of whole-model batches.  The ids live on the device (out_dev: row i's list, entry step0 + t written by
    // tick t since the last batch_set); what the host needs at a swap it reads then: the token tick t evaluated is entry step0 + t - 1 (or
    // tok0[i], the host value of the last batch_set, for entry -1).
    std::vector<uint32_t> pos_set, tok0, pending;
    bool tok0_known = false;
    uint32_t step0 = 0, ticks = 0, drained = 0;   // ticks since the last batch_set / of them recorded in the pods' token histories
    bool collecting = false;                      // lh_batch_decode: keep every id a row produces across the resets of the device lists
    std::vector<std::vector<uint32_t>> gen;
    // lh_batch_feed: the passes' row tables, token ids and query blocks (one device buffer, grown on demand) and split-T partials for a 64-row pass
    char* feed_dev = nullptr;
    size_t feed_cap = 0;
    float* feed_part = nullptr;
    BatchSpec* spec = nullptr;     // lh_batch_decode_lookup: device state + the captured pass
    // Prefix sharing (lh_batch_fork).  Host state: pod i is a member of group sh_gid[i] (SH_NONE: of none) of shared length sh_len[i];
    // the invariant of a member is "my cache rows [0, len) are byte-equal to every other member's" (share_written enforces it).
    // Device: the block table the shared tick kernel reads (batched, split partials), the table last sent, and what the captured tick was captured for.
    static constexpr uint32_t SH_NONE = 0xFFFFFFFFu;
    std::vector<uint32_t> sh_gid, sh_len;
    uint32_t sh_next_gid = 0;
    ShareTable* share_dev = nullptr;
    ShareTable share_sent;         // (set to "no block" where share_dev is allocated)
    uint32_t share_sent_blocks = 0;
    bool shared = false;           // the tick takes k_attention_split_shared (some block in the table, LLAMAHIP_SHARE_ROW_ATTN unset)
    uint32_t share_qb = 0;
    float* logits() const { return batched || B == 1 ? pods[0]->logits : logits_own; }
};

// ---- prefix sharing: group state (host only) ---------------------------------------------------------------------------------------------------
static void share_set(Batch* b, uint32_t pod, uint32_t gid, uint32_t len) {
    b->sh_gid[pod] = gid; b->sh_len[pod] = len;
    b->pods[pod]->share_len = len; b->pods[pod]->share_broken = false;
}
// pod leaves its group; a group of one member dissolves
static void share_leave(Batch* b, uint32_t pod) {
    const uint32_t gid = b->sh_gid[pod];
    if (gid == Batch::SH_NONE) return;
    share_set(b, pod, Batch::SH_NONE, 0);
    uint32_t n = 0, last = 0;
    for (uint32_t i = 0; i < b->B; ++i) if (b->sh_gid[i] == gid) { ++n; last = i; }
    if (n == 1) share_set(b, last, Batch::SH_NONE, 0);
}
// THE predicate: something writes pod's cache from position pos_lo on
static void share_written(Batch* b, uint32_t pod, uint32_t pos_lo) {
    if (b->sh_gid[pod] != Batch::SH_NONE && pos_lo < b->sh_len[pod]) share_leave(b, pod);
}
// Evals on the pods' own plans since the batch last looked (Plan::share_broken: a solo feed pass, the re-fed Eval of a context swap, lh_llama_eval)
static void share_sync(Batch* b) {
    for (uint32_t i = 0; i < b->B; ++i) if (b->pods[i]->share_broken) share_leave(b, i);
}
static void share_info(Batch* b, uint32_t* group, uint32_t* len) {
    share_sync(b);
    for (uint32_t i = 0; i < b->B; ++i) {
        uint32_t lo = i;
        if (b->sh_gid[i] != Batch::SH_NONE) for (uint32_t j = 0; j < i; ++j) if (b->sh_gid[j] == b->sh_gid[i]) { lo = j; break; }
        group[i] = lo; len[i] = b->sh_len[i];
    }
}

// the kernels of one tick, in stream order
static int batch_enqueue_tick(Batch* b, const float* x_in, float* x_out) {
    lh_ctx* ctx = b->ctx;
    Plan* p0 = b->pods[0];
    const ModelDesc& m = p0->md;
    const uint32_t B = b->B;
    int rc;
    if (b->batched) {
        BatchCtx bc = {b->rows_dev, b->tok_dev, b->attn_part};
        if (b->shared) {   // some pods share a prefix: the shared tick kernel on the table share_prepare sent (with no block: exactly the launches of a batch that never forked)
            bc.share = b->share_dev; bc.share_qb = b->share_qb; bc.share_blocks = b->share_sent_blocks;
            for (uint32_t i = 0; i < B; ++i) bc.share_rows += b->share_sent.row_block[i] != SHARE_NO_BLOCK;
        }
        if ((rc = plan_eval(p0, nullptr, x_in, x_out, B, 0, false, &bc))) return rc;
    } else {
        for (uint32_t i = 0; i < B; ++i) {
            Plan* p = b->pods[i];
            if ((rc = enqueue_decode(p, b->sp_dev + i, x_in ? x_in + (size_t)i * m.d : nullptr, x_out ? x_out + (size_t)i * m.d : nullptr, 0, nullptr, b->tok_dev + i))) return rc;
            if (m.last_stage() && B > 1) LH_HIP(ctx, hipMemcpyAsync(b->logits_own + (size_t)i * m.V, p->logits, (size_t)m.V * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    if (m.last_stage() && b->sampling) {
        // SampleTopPTopK per row (llama.go:455-707) on the row's own ring / draw counter; the rows' step parameters carry the output index.
        // One launch, a workgroup per row (they run on separate CUs); the per-row launches stay as the A/B switch the tests compare against.
        if (!b->per_pod) {
            if ((rc = sample_pods_launch(ctx, b->logits(), m.V, B, nullptr, b->ss_dev, b->ring_dev, b->ring_cap, b->sp_dev, b->out_dev, b->out_cap, b->ids_dev, b->smp_topk))) return rc;
        } else {
            for (uint32_t i = 0; i < B; ++i) {
                LH_TRACE("%s", b->smp_topk <= 64 ? "k_sample_small" : "k_sample");
                if ((rc = sample_launch(ctx, b->logits() + (size_t)i * m.V, m.V, b->ss_dev + i, b->ring_dev + (size_t)i * b->ring_cap, b->sp_dev + i,
                                        b->out_dev + (size_t)i * b->out_cap, nullptr, nullptr, nullptr, nullptr, 1, b->smp_topk)))
                    return rc;
            }
        }
        LH_LAUNCH(k_batch_from_sp, dim3(1), dim3(64), 0, ctx->stream, b->rows_dev, b->tok_dev, b->ids_dev, (const StepParams*)b->sp_dev, B);
    } else if (m.last_stage()) {
        LH_LAUNCH(k_batch_argmax, dim3(B), dim3(1024), 0, ctx->stream, (const float*)b->logits(), m.V, b->rows_dev, b->tok_dev, b->ids_dev, b->out_dev, b->out_cap,
                           b->sp_dev, 1);
    } else {
        LH_LAUNCH(k_batch_advance, dim3(1), dim3(64), 0, ctx->stream, b->rows_dev, b->sp_dev, B);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

// One tick on the stream: the first one eagerly (it sets kernel attributes and makes the allocations a capture must not make), then a
// captured graph, re-captured when an address it holds has changed.
static int batch_tick_unchecked(Batch* b, const float* x_in, float* x_out);
static int batch_swap(Batch* b);
static int share_prepare(Batch* b);
static int batch_tick(Batch* b, const float* x_in, float* x_out) {
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    // a tick evaluates row i at position pos[i]: RoPE table row, KV append and the attention's key range all index by it (Eval's
    // pastCount + N <= CtxSize, checked like plan_eval / lh_llama_stage do)
    if (!b->pos_known) LH_FAIL(ctx, LH_EINVAL, "lh_batch: tick before lh_batch_set / lh_batch_prompt placed the rows");
    bool full = false;
    for (uint32_t i = 0; i < b->B; ++i) full = full || b->pos[i] >= m.ctx;
    int rc;
    if (full && (rc = batch_swap(b))) return rc;   // whole-model batches swap context like server.Do; a stage's batch fails here
    share_sync(b);
    for (uint32_t i = 0; i < b->B; ++i) share_written(b, i, b->pos[i]);   // the tick appends row i's K / V at pos[i]: below a shared length the pod leaves its group
    rc = batch_tick_unchecked(b, x_in, x_out);
    if (rc == 0) { for (uint32_t i = 0; i < b->B; ++i) b->pos[i] += 1; b->ticks += 1; }
    return rc;
}
static int batch_tick_unchecked(Batch* b, const float* x_in, float* x_out) {
    lh_ctx* ctx = b->ctx;
    Plan* p0 = b->pods[0];
    int rc;
    const char* pp = getenv("LLAMAHIP_SAMPLE_PER_POD");
    b->per_pod = pp && pp[0] == '1';
    if ((rc = share_prepare(b))) return rc;   // the block table of the pods that share a prefix, re-sent when it changed (outside the captured graph)
    const Batch::TickKey key = {x_in, x_out, ctx->splitk_gen, b->scratch_gen(), b->smp_gen, b->sampling, b->per_pod, b->shared, b->shared ? b->share_qb : 0, f16_stream_key(p0)};
    f16_stream_sync(b->tick, &b->f16_seen, key.f16_stream);
    return b->tick.run(ctx, p0->use_graph, 0, key, " (batch tick)", [&] { return batch_enqueue_tick(b, x_in, x_out); });
}

static void batch_spec_free(Batch* b);
static void batch_free(Batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    b->tick.drop();
    batch_spec_free(b);
    void* bufs[] = {b->rows_dev, b->tok_dev, b->ids_dev, b->out_dev, b->sp_dev, b->logits_own, b->attn_part, b->ss_dev, b->ring_dev, b->feed_dev, b->feed_part, b->share_dev};
    for (void* q : bufs) if (q) hipFree(q);
    delete b;
}

// positions (and, tokens != nullptr, token ids) of the next tick from host values; the tick counter restarts at step0
static int batch_set(Batch* b, const uint32_t* tokens, const uint32_t* past, uint32_t step0 = 0) {
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    BatchSetArgs v = {};
    for (uint32_t i = 0; i < b->B; ++i) {
        // past == ctx is a legal resting place (a prompt that filled the window, Eval's pastCount + N <= CtxSize): a tick from there is refused by batch_tick
        if (past[i] > m.ctx) LH_FAIL(ctx, LH_EINVAL, "lh_batch_set: row %u at position %u outside the context window of %u", i, past[i], m.ctx);
        if (tokens && tokens[i] >= m.V) LH_FAIL(ctx, LH_EINVAL, "lh_batch_set: token id %u of row %u outside the vocabulary of %u", tokens[i], i, m.V);
        v.pos[i] = past[i];
        v.tok[i] = tokens ? tokens[i] : 0;
    }
    LH_LAUNCH(k_batch_set, dim3(1), dim3(64), 0, ctx->stream, b->rows_dev, b->tok_dev, b->B, tokens ? 1 : 0, v, b->sp_dev, step0);
    LH_HIP(ctx, hipGetLastError());
    b->pos.assign(past, past + b->B);
    b->pos_known = true;
    b->pos_set = b->pos;
    b->tok0_known = tokens != nullptr;
    if (tokens) b->tok0.assign(tokens, tokens + b->B);
    b->step0 = step0; b->ticks = 0; b->drained = 0;
    return 0;
}

// Waits for the stream and brings the host up to date with what the ticks since the last batch_set did: the token every tick evaluated goes
// into its pod's history (Plan::hist), the ids produced into b->gen (lh_batch_decode), the rows' pending tokens into b->pending.
static int batch_drain(Batch* b) {
    lh_ctx* ctx = b->ctx;
    const uint32_t B = b->B, n_out = b->step0 + b->ticks;
    const ModelDesc& m = b->pods[0]->md;
    if (!m.last_stage()) LH_FAIL(ctx, LH_EINVAL, "lh_batch: only the last stage knows the ids");
    std::vector<uint32_t> out((size_t)B * std::max(n_out, 1u));
    if (n_out) LH_HIP(ctx, hipMemcpy2DAsync(out.data(), (size_t)n_out * 4, b->out_dev, (size_t)b->out_cap * 4, (size_t)n_out * 4, B, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    b->pending.assign(B, Plan::HIST_UNKNOWN);
    for (uint32_t i = 0; i < B; ++i) {
        auto evaluated = [&](uint32_t t) -> uint32_t {   // the token tick t evaluated
            if (b->step0 + t >= 1) return out[(size_t)i * n_out + b->step0 + t - 1];
            return b->tok0_known ? b->tok0[i] : Plan::HIST_UNKNOWN;
        };
        for (uint32_t t = b->drained; t < b->ticks; ++t) {
            b->pods[i]->record(b->pos_set[i] + t, evaluated(t));
            if (b->collecting) b->gen[i].push_back(out[(size_t)i * n_out + b->step0 + t]);
        }
        b->pending[i] = evaluated(b->ticks);
    }
    b->drained = b->ticks;
    return 0;
}

// The rows whose window is full swap context (server.go:160-172), each on its own plan and cache like its prompt ran: the run of
// (position - keep) / 2 tokens is re-fed as ONE Eval at position keep, and the row's pending token then takes the next tick at the position
// behind it - together exactly the reference's swap Eval (the pending token last in it), cut in two at its last row.
static int batch_swap(Batch* b) {
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    if (!m.first_stage() || !m.last_stage())
        LH_FAIL(ctx, LH_EINVAL, "lh_batch: a row has left the context window of %u (the context swap of a layer shard is driven by the pipeline, not by a stage)", m.ctx);
    int rc;
    if ((rc = batch_drain(b))) return rc;
    std::vector<uint32_t> newpos = b->pos, refeed;
    for (uint32_t i = 0; i < b->B; ++i) {
        if (b->pos[i] < m.ctx) continue;
        Plan* p = b->pods[i];
        if (p->keep >= m.ctx) LH_FAIL(ctx, LH_EINVAL, "context swap: KeepCount %u leaves no room in a window of %u", p->keep, m.ctx);
        if (b->pending[i] == Plan::HIST_UNKNOWN || !swap_refeed_tokens(p, b->pos[i], b->pending[i], &refeed))
            LH_FAIL(ctx, LH_EINVAL, "lh_batch: row %u has left the context window of %u and the tokens of its window are not known to the batch (run its prompt through lh_batch_prompt)", i, m.ctx);
        if (!refeed.empty() && (rc = plan_eval(p, refeed.data(), nullptr, nullptr, (uint32_t)refeed.size(), p->keep, true))) return rc;
        newpos[i] = p->keep + (uint32_t)refeed.size();
    }
    const std::vector<uint32_t> toks = b->pending;   // (batch_set overwrites b->tok0 from it)
    return batch_set(b, toks.data(), newpos.data(), 0);
}

// ---- lh_batch_feed: llama.Eval for any subset of the pods, packed into shared weight passes --------------------------------------------
// The schedule (feed_schedule.h) is a fixed partition of the fed rows; this function executes exactly what it returns.  A batched pass is one
// plan_eval on pod 0's plan over a row table of its own: the rows of one segment name the same cache at consecutive positions, the wq|wk|wv
// launch appends every row's K / V before the attention launch reads them, so the segment is a causal chunk.  Host bookkeeping as batch_swap:
// batch_drain, the per-row work, one batch_set (step0 = 1: entry 0 of every output list holds the row's pending token, as lh_batch_prompt leaves it).
static constexpr uint32_t FEED_SOLO_MIN = 129;   // the first length that leaves the single stream pass (fp32: 128 rows).  NOT yet set by measurement:
                                                 // DESIGN 3h; sweep with tools/bench_feed.py --sweep, override with LLAMAHIP_FEED_SOLO_MIN
static constexpr uint32_t FEED_QB = 4;           // query rows per attention block (LLAMAHIP_FEED_QB: 2, 4, 8).  Measured, a 64-token chunk behind 1984 keys, 8 layers:
                                                 // 3.9-4.2 ms at 4 (two workgroups per CU), 4.5-4.7 at 8 (one), 4.6-4.7 at 2; per-row kernels 6.6-6.8 (profiles/feed_ragged.txt)
static uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* e = getenv(name);
    return (e && *e) ? (uint32_t)strtoul(e, nullptr, 10) : dflt;
}

// ---- prefix sharing: the tick's block table ---------------------------------------------------------------------------------------------------------
// Before a tick is enqueued the batch derives the table from the pods' group state (share_schedule.h: a pure function, B <= 64 rows), compares it with
// the table last sent and re-sends it on change (k_share_set, the table as kernel arguments, in stream order in front of the tick: the captured graph
// reads it from a fixed address, so a changed table needs no new capture).  Only "no block" <-> "some block" changes the tick's launches (TickKey::shared).
// Switches, read per tick: LLAMAHIP_SHARE_ROW_ATTN=1 (the per-row kernels: the A/B switch and the tests' reference), LLAMAHIP_SHARE_QB, LLAMAHIP_SHARE_MIN.
static constexpr uint32_t SHARE_QB = 4;    // rows per block (LLAMAHIP_SHARE_QB: 2, 4, 8).  Measured (profiles/shared_prefix.txt, 7B fp32, ctx 2048): 4 beats 8 in every case - 64 pods
                                           // behind 1920 shared keys 18.15 ms per tick at 4 (two workgroups per CU), 20.71 at 8 (one), 29.19 on the per-row kernels
static constexpr uint32_t SHARE_MIN = 2;   // smallest group that gets blocks (LLAMAHIP_SHARE_MIN).  Measured: 16 pairs behind 1024 / 1920 keys 10.29 / 12.79 ms against 11.73 / 16.40
                                           // per-row.  Behind 256 keys every group size loses (pairs 4.6 %, larger groups 0.6-1.6 %): a matter of the length, not of this value
static int share_prepare(Batch* b) {
    lh_ctx* ctx = b->ctx;
    b->shared = false;
    if (!b->share_dev) return 0;   // row-by-row batches and plans without split partials (ctx <= 256, hd != 128): ticks run as they always did
    const char* ra = getenv("LLAMAHIP_SHARE_ROW_ATTN");
    const bool row_attn = ra && ra[0] == '1';
    const uint32_t qb = env_u32("LLAMAHIP_SHARE_QB", SHARE_QB), min_rows = env_u32("LLAMAHIP_SHARE_MIN", SHARE_MIN);
    if (qb != 2 && qb != 4 && qb != 8) LH_FAIL(ctx, LH_EINVAL, "lh_batch: LLAMAHIP_SHARE_QB = %u (2, 4 or 8)", qb);
    ShareTable t;
    memset(&t, 0, sizeof t);
    for (uint32_t j = 0; j < SHARE_ROWS_MAX; ++j) t.row_block[j] = SHARE_NO_BLOCK;
    int nb = 0;
    if (!row_attn) {
        uint32_t group[SHARE_ROWS_MAX], len[SHARE_ROWS_MAX];
        share_info(b, group, len);
        nb = share_schedule(group, len, b->B, qb, min_rows, t.blocks, SHARE_BLOCKS_MAX, t.row_block);
        if (nb < 0) LH_FAIL(ctx, LH_EINVAL, "lh_batch: the sharing groups of the batch are inconsistent (internal)");
    }
    if (memcmp(&t, &b->share_sent, sizeof t) != 0) {
        LH_TRACE("share_table/b%u", (uint32_t)nb);
        LH_LAUNCH(k_share_set, dim3(1), dim3(512), 0, ctx->stream, b->share_dev, t);
        LH_HIP(ctx, hipGetLastError());
        b->share_sent = t; b->share_sent_blocks = (uint32_t)nb;
    }
    b->shared = nb > 0; b->share_qb = qb;
    return 0;
}

// sample: lh_batch_feed_sample - the same feed on a batch whose ticks sample; the fed pods' rings (k_feed_ring) and the id behind a pod's last row
// (the pods sampler in place of the argmax) are all that differs.
static int batch_feed(Batch* b, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past, const uint32_t* flags, bool sample, uint32_t* ids_host,
                      float* logits_last_host, float* logits_rows_host) {
    lh_ctx* ctx = b->ctx;
    Plan* p0 = b->pods[0];
    const ModelDesc& m = p0->md;
    const uint32_t B = b->B;
    const char* who = sample ? "lh_batch_feed_sample" : "lh_batch_feed";
    // ---- everything is checked before anything is enqueued or any host state moves
    if (!m.first_stage() || !m.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "%s needs whole-model pods (a layer shard's prompts are driven by the pipeline)", who);
    if (sample && !b->sampling) LH_FAIL(ctx, LH_EINVAL, "lh_batch_feed_sample: the batch has no sampler set (lh_batch_feed feeds a greedy batch)");
    if (!sample && b->sampling) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_batch_feed: the batch has a sampler set (sampler rings across a feed are out of scope; lh_batch_set_sampler(NULL) first)");
    uint64_t total = 0;
    for (uint32_t i = 0; i < B; ++i) {
        const uint32_t n = n_tokens[i];
        if (!n) {
            if (!b->pos_known) LH_FAIL(ctx, LH_EINVAL, "%s: the first feed of a fresh batch must feed every row (row %u has no position yet)", who, i);
            continue;
        }
        if (!tokens || !tokens[i]) LH_FAIL(ctx, LH_EINVAL, "%s: row %u has %u tokens to feed and no token array", who, i, n);
        if (!past || (uint64_t)past[i] + n > m.ctx) LH_FAIL(ctx, LH_EINVAL, "%s: row %u: past %u + n %u exceeds the context window of %u", who, i, past ? past[i] : 0u, n, m.ctx);
        for (uint32_t j = 0; j < n; ++j)
            if (tokens[i][j] >= m.V) LH_FAIL(ctx, LH_EINVAL, "%s: row %u: token id %u at index %u outside the vocabulary of %u", who, i, tokens[i][j], j, m.V);
        total += n;
    }
    if (!total) LH_FAIL(ctx, LH_EINVAL, "%s: no row is fed", who);
    int rc;
    if (sample) {
        bool pending = false;
        for (uint32_t i = 0; i < B; ++i) {
            const uint32_t fl = (flags && n_tokens[i]) ? flags[i] : 0u;
            if (fl & ~(uint32_t)(LH_FEED_NEW | LH_FEED_PENDING)) LH_FAIL(ctx, LH_EINVAL, "lh_batch_feed_sample: row %u: unknown flag bits 0x%x", i, fl);
            if ((fl & LH_FEED_NEW) && (fl & LH_FEED_PENDING)) LH_FAIL(ctx, LH_EINVAL, "lh_batch_feed_sample: row %u: LH_FEED_NEW and LH_FEED_PENDING exclude each other", i);
            pending = pending || (fl & LH_FEED_PENDING);
        }
        if (pending) {   // the pod's position and pending id, as the host knows them once the ticks so far are read (a stream wait and the host mirror's histories: neither device state nor positions move)
            if (!b->pos_known) LH_FAIL(ctx, LH_EINVAL, "lh_batch_feed_sample: LH_FEED_PENDING on a fresh batch (no row has a pending id yet)");
            if ((rc = batch_drain(b))) return rc;
            for (uint32_t i = 0; i < B; ++i) {
                if (!n_tokens[i] || !(flags[i] & LH_FEED_PENDING)) continue;
                if (past[i] != b->pos[i] || b->pending[i] == Plan::HIST_UNKNOWN || tokens[i][0] != b->pending[i])
                    LH_FAIL(ctx, LH_EINVAL, "lh_batch_feed_sample: row %u: LH_FEED_PENDING needs past = the row's position %u and tokens[0] = its pending id (got past %u, id %u)", i,
                            b->pos[i], past[i], tokens[i][0]);
            }
        }
    }
    const uint32_t solo_min = env_u32("LLAMAHIP_FEED_SOLO_MIN", FEED_SOLO_MIN), qb = env_u32("LLAMAHIP_FEED_QB", FEED_QB);
    if (qb != 2 && qb != 4 && qb != 8) LH_FAIL(ctx, LH_EINVAL, "%s: LLAMAHIP_FEED_QB = %u (2, 4 or 8)", who, qb);
    const char* ra = getenv("LLAMAHIP_FEED_ROW_ATTN");
    const bool row_attn = ra && ra[0] == '1';
    uint64_t sizes_ok = 0;   // the row counts that may share one weight pass on this plan
    if (b->batched)
        for (uint32_t n = 2; n <= FEED_PASS_ROWS; ++n) if (plan_batch_rows_ok(p0, n)) sizes_ok |= 1ull << (n - 1);
    FeedSchedule fs;
    feed_schedule(n_tokens, past, B, solo_min, qb, sizes_ok, &fs);
    // ---- the passes' tables: [BatchRow x rows | token id x rows | AttnBlock x blocks] per batched pass, one upload through the pinned staging buffer
    std::vector<uint64_t> row_off(B, 0);   // logits_rows_host, and the token table of a sampled feed: every fed row, pods in index order
    for (uint32_t i = 1; i < B; ++i) row_off[i] = row_off[i - 1] + n_tokens[i - 1];
    std::vector<size_t> pass_off(fs.passes.size(), 0);
    size_t bytes = 0;
    for (size_t k = 0; k < fs.passes.size(); ++k) {
        const lh_feed_pass& ps = fs.passes[k];
        if (ps.kind != LH_FEED_BATCHED) continue;
        pass_off[k] = bytes;
        bytes += (sizeof(BatchRow) * ps.rows + 4 * (size_t)ps.rows + sizeof(AttnBlock) * ps.nblk + 15) & ~(size_t)15;
    }
    const size_t pass_bytes = bytes;
    // a sampled feed: [FeedRingSeg x segments | SampleJob x segments (per pass, from its first segment's index: the segments that END in it) | every fed token]
    const size_t n_segs = fs.segs.size(), o_rseg = bytes, o_jobs = o_rseg + sizeof(FeedRingSeg) * n_segs, o_toks = o_jobs + sizeof(SampleJob) * n_segs;
    std::vector<uint32_t> n_end(fs.passes.size(), 0);
    std::vector<SampleJob> jobs(sample ? n_segs : 0);   // (kept on the host too: a solo pass reuses the staging buffer)
    if (sample) bytes = (o_toks + 4 * (size_t)total + 15) & ~(size_t)15;
    if (pass_bytes && (rc = plan_ensure_rows(p0, FEED_PASS_ROWS))) return rc;   // (the captured tick re-captures on scratch_gen)
    if (bytes) {
        if ((rc = ensure_staging(ctx, bytes))) return rc;
        if ((rc = grow(ctx, &b->feed_dev, &b->feed_cap, bytes))) return rc;
        if (pass_bytes && p0->attn_part && !b->feed_part)
            LH_HIP(ctx, hipMalloc((void**)&b->feed_part, 4 * (size_t)FEED_PASS_ROWS * m.H * ((m.ctx + ATT_TC - 1) / ATT_TC) * (m.hd + 2)));
    }
    // what the ticks so far did goes into the pods' histories (and waits for the stream: the staging buffer is free)
    if (b->pos_known) { if ((rc = batch_drain(b))) return rc; }
    else LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) {
        for (size_t k = 0; k < fs.passes.size(); ++k) {
            const lh_feed_pass& ps = fs.passes[k];
            if (ps.kind != LH_FEED_BATCHED) continue;
            BatchRow* hr = (BatchRow*)(ctx->staging + pass_off[k]);
            uint32_t* ht = (uint32_t*)(hr + ps.rows);
            AttnBlock* hb = (AttnBlock*)(ht + ps.rows);
            for (uint32_t s = ps.seg0; s < ps.seg0 + ps.nseg; ++s) {
                const lh_feed_seg& sg = fs.segs[s];
                const Plan* pp = b->pods[sg.pod];
                for (uint32_t j = 0; j < sg.n; ++j) {
                    hr[sg.row0 + j] = BatchRow{pp->md.kc, pp->md.vc, sg.pos0 + j, 0u};
                    ht[sg.row0 + j] = tokens[sg.pod][sg.pos0 - past[sg.pod] + j];
                }
            }
            uint32_t w = 0;   // the blocks of one row first (they take the QB = 1 instantiation), then the others, each group in schedule order
            for (int one = 1; one >= 0; --one)
                for (uint32_t q = 0; q < ps.nblk; ++q)
                    if ((fs.blocks[ps.blk0 + q].n == 1) == (one == 1)) hb[w++] = AttnBlock{fs.blocks[ps.blk0 + q].row0, fs.blocks[ps.blk0 + q].n};
        }
        if (sample) {
            FeedRingSeg* hs = (FeedRingSeg*)(ctx->staging + o_rseg);
            uint32_t* ht = (uint32_t*)(ctx->staging + o_toks);
            for (uint32_t i = 0; i < B; ++i)
                for (uint32_t j = 0; j < n_tokens[i]; ++j) ht[row_off[i] + j] = tokens[i][j];
            for (size_t k = 0; k < fs.passes.size(); ++k) {
                const lh_feed_pass& ps = fs.passes[k];
                for (uint32_t s = ps.seg0; s < ps.seg0 + ps.nseg; ++s) {
                    const lh_feed_seg& sg = fs.segs[s];
                    const uint32_t fl = flags ? flags[sg.pod] : 0u, t0 = sg.pos0 - past[sg.pod];
                    const uint32_t skip = (t0 == 0 && (fl & LH_FEED_PENDING)) ? 1u : 0u;   // the pending id is in the ring already
                    hs[s] = FeedRingSeg{sg.pod, (uint32_t)row_off[sg.pod] + t0 + skip, sg.n - skip, (t0 == 0 && (fl & LH_FEED_NEW)) ? 1u : 0u};
                    if (t0 + sg.n == n_tokens[sg.pod])   // a solo pass hands its last row to the sampler as row 0
                        jobs[ps.seg0 + n_end[k]++] = SampleJob{sg.pod, ps.kind == LH_FEED_SOLO ? 0u : sg.row0 + sg.n - 1};
                }
            }
            memcpy(ctx->staging + o_jobs, jobs.data(), sizeof(SampleJob) * n_segs);
        }
        LH_HIP(ctx, hipMemcpyAsync(b->feed_dev, ctx->staging, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    // a batched pass runs on pod 0's plan over a row table and writes OTHER pods' caches, so the batch applies the sharing predicate here (a solo pass also
    // notes itself on its pod's plan): a pod fed below its group's shared length leaves the group
    for (uint32_t i = 0; i < B; ++i) if (n_tokens[i]) share_written(b, i, past[i]);
    // a sampled pass: the rings of its segments in front of it, one sampler launch over the pods whose feed ends in it behind it
    auto pass_rings = [&](const lh_feed_pass& ps) -> int {
        return feed_ring_launch(ctx, (const FeedRingSeg*)(b->feed_dev + o_rseg) + ps.seg0, ps.nseg, (const uint32_t*)(b->feed_dev + o_toks), b->ss_dev, b->ring_dev, b->ring_cap);
    };
    auto pass_sample = [&](size_t k, const float* lg) -> int {
        const lh_feed_pass& ps = fs.passes[k];
        if (!n_end[k]) return 0;
        int r = sample_pods_launch(ctx, lg, m.V, n_end[k], (const SampleJob*)(b->feed_dev + o_jobs) + ps.seg0, b->ss_dev, b->ring_dev, b->ring_cap, b->sp_dev, b->out_dev,
                                   b->out_cap, b->ids_dev, b->smp_topk);
        if (r) return r;
        const SampleJob* hj = jobs.data() + ps.seg0;
        for (uint32_t e = 0; e < n_end[k]; ++e)
            LH_HIP(ctx, hipMemcpyAsync(b->tok_dev + hj[e].pod, b->ids_dev + hj[e].pod, 4, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    };
    // rows [r0, r0 + n) of `lg` are tokens tok0.. of pod's feed: the copies the caller asked for, and the pod's next id behind its last row
    auto rows_done = [&](uint32_t pod, uint32_t tok0, uint32_t n, const float* lg) -> int {
        if (logits_rows_host)
            LH_HIP(ctx, hipMemcpyAsync(logits_rows_host + (row_off[pod] + tok0) * m.V, lg, (size_t)n * m.V * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (tok0 + n != n_tokens[pod]) return 0;   // (the pod's feed continues in the next pass)
        const float* last_row = lg + (size_t)(n - 1) * m.V;
        if (!sample) {   // (a sampled pass draws the ids of all its ending pods in one launch: pass_sample)
            LH_LAUNCH(k_argmax_advance, dim3(1), dim3(1024), 0, ctx->stream, last_row, m.V, (StepParams*)nullptr, b->out_dev + (size_t)pod * b->out_cap, b->ids_dev + pod, 0);
            LH_HIP(ctx, hipMemcpyAsync(b->tok_dev + pod, b->ids_dev + pod, 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (logits_last_host) LH_HIP(ctx, hipMemcpyAsync(logits_last_host + (size_t)pod * m.V, last_row, (size_t)m.V * 4, hipMemcpyDeviceToHost, ctx->stream));
        return 0;
    };
    for (size_t k = 0; k < fs.passes.size(); ++k) {
        const lh_feed_pass& ps = fs.passes[k];
        if (ps.kind == LH_FEED_SOLO) {   // an Eval on the pod's own plan (it records its tokens itself)
            const lh_feed_seg& sg = fs.segs[ps.seg0];
            Plan* pp = b->pods[sg.pod];
            const uint32_t tok0 = sg.pos0 - past[sg.pod];
            LH_TRACE("feed_pass/solo/n%u", sg.n);
            if (sample && (rc = pass_rings(ps))) return rc;
            if ((rc = plan_eval(pp, tokens[sg.pod] + tok0, nullptr, nullptr, sg.n, sg.pos0, logits_rows_host == nullptr))) return rc;
            // (last_row_only leaves the last row in its usual place, row n - 1; the rows in front of it are then not the caller's)
            if (logits_rows_host) { if ((rc = rows_done(sg.pod, tok0, sg.n, pp->logits))) return rc; }
            else if ((rc = rows_done(sg.pod, tok0 + sg.n - 1, 1, pp->logits + (size_t)(sg.n - 1) * m.V))) return rc;
            if (sample && (rc = pass_sample(k, pp->logits + (size_t)(sg.n - 1) * m.V))) return rc;
            continue;
        }
        char* base = b->feed_dev + pass_off[k];
        BatchCtx bc = {};
        bc.rows = (const BatchRow*)base;
        bc.tok_dev = (const uint32_t*)(base + sizeof(BatchRow) * ps.rows);
        bc.attn_part = p0->attn_part ? b->feed_part : nullptr;
        for (uint32_t s = ps.seg0; s < ps.seg0 + ps.nseg; ++s) {
            const lh_feed_seg& sg = fs.segs[s];
            bc.max_T = std::max(bc.max_T, sg.pos0 + sg.n);
            for (uint32_t j = 0; j < sg.n; ++j) b->pods[sg.pod]->record(sg.pos0 + j, tokens[sg.pod][sg.pos0 - past[sg.pod] + j]);
        }
        if (!row_attn) {
            bc.blocks = (const AttnBlock*)(base + (sizeof(BatchRow) + 4) * (size_t)ps.rows); bc.n_blocks = ps.nblk; bc.qb = qb;
            for (uint32_t q = 0; q < ps.nblk; ++q) bc.n_blocks1 += fs.blocks[ps.blk0 + q].n == 1;
        }
        LH_TRACE("feed_pass/batched/n%u", ps.rows);
        if (sample && (rc = pass_rings(ps))) return rc;
        if ((rc = plan_eval(p0, nullptr, nullptr, nullptr, ps.rows, 0, false, &bc))) return rc;
        for (uint32_t s = ps.seg0; s < ps.seg0 + ps.nseg; ++s) {   // before the next pass overwrites p0->logits
            const lh_feed_seg& sg = fs.segs[s];
            if ((rc = rows_done(sg.pod, sg.pos0 - past[sg.pod], sg.n, p0->logits + (size_t)sg.row0 * m.V))) return rc;
        }
        if (sample && (rc = pass_sample(k, p0->logits))) return rc;
    }
    LH_LAUNCH(k_batch_feed_heads, dim3(1), dim3(64), 0, ctx->stream, b->out_dev, b->out_cap, (const uint32_t*)b->tok_dev, B);
    LH_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> newpos(B);
    for (uint32_t i = 0; i < B; ++i) newpos[i] = n_tokens[i] ? past[i] + n_tokens[i] : b->pos[i];
    if ((rc = batch_set(b, nullptr, newpos.data(), 1))) return rc;
    std::vector<uint32_t> ids(B);
    if (ids_host) LH_HIP(ctx, hipMemcpyAsync(ids.data(), b->ids_dev, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ids_host)
        for (uint32_t i = 0; i < B; ++i) if (n_tokens[i]) ids_host[i] = ids[i];
    return 0;
}

// ---- lookup-draft speculative decoding (kernels_spec.h) -----------------------------------------------------------------------------
// A pass = the batched plan_eval over a row table whose R rows all name THIS plan's cache at consecutive positions (a causal chunk, as a fed
// prompt chunk of lh_batch_feed), k_batch_argmax over the R logits rows, k_spec_accept.  Everything a pass depends on lives in device memory, and
// on the row-table route the attention launches are sized by the window, so a pass is captured once and replayed.
// The sampled route (lh_llama_decode_sample_lookup) differs in two launches: k_sample_rows / k_sample_small_rows instead of k_batch_argmax, and
// the accept step commits the plan's ring and draw counter (ss_dev / ring_dev); its ids land behind the first sample, at out_tokens_dev + 1.
struct Spec {
    SpecState* st = nullptr;
    StepParams* sp = nullptr;          // {pending token, its position}: what the one-row pass at the window's end reads
    BatchRow* rows = nullptr;          // [SPEC_ROWS_MAX]
    uint32_t* tok = nullptr;           // [SPEC_ROWS_MAX] pending, draft, filler
    uint32_t* arg = nullptr;           // [SPEC_ROWS_MAX] greedy ids of the last pass
    uint32_t* win = nullptr;           // [ctx + 1] the window's tokens, the pending one last
    uint32_t* corpus = nullptr;
    uint32_t corpus_cap = 0;
    uint16_t* trace = nullptr;
    uint32_t trace_cap = 0;
    float* part = nullptr;             // split-T attention partials for SPEC_ROWS_MAX rows (plans with ctx > 256)
    bool smp = false;                  // the passes sample (set by the entry points before they enqueue a pass)
    // the captured pass (warm bit R: a pass of R rows) and what it holds by value
    struct Key {
        uint32_t R, trace_cap;
        SpecLookup lp;
        uint32_t* out;
        uint16_t* trace;
        uint64_t splitk_gen, scratch_gen;
        uint32_t smp, smp_small;       // sampled route: the kernel variant (topK <= 64 or not) and the ring pointer
        uint32_t* ring;
        uint64_t f16_stream;           // f16_stream_key
    };
    CapturedGraph<Key> pass;
    uint64_t f16_seen = 0;
};
static void spec_free(Plan* p) {
    Spec* s = p->spec;
    if (!s) return;
    s->pass.drop();
    void* bufs[] = {s->st, s->sp, s->rows, s->tok, s->arg, s->win, s->corpus, s->trace, s->part};
    for (void* q : bufs) if (q) hipFree(q);
    delete s;
    p->spec = nullptr;
}
// every allocation of the route, outside any capture
static int spec_ensure(Plan* p, uint32_t n_corpus, uint32_t n_trace) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    if (!p->spec) p->spec = new Spec();
    Spec* s = p->spec;
    if (!s->st) {
        LH_HIP(ctx, hipMalloc((void**)&s->st, sizeof(SpecState)));
        LH_HIP(ctx, hipMalloc((void**)&s->sp, sizeof(StepParams)));
        LH_HIP(ctx, hipMalloc((void**)&s->rows, sizeof(BatchRow) * SPEC_ROWS_MAX));
        LH_HIP(ctx, hipMalloc((void**)&s->tok, 4 * SPEC_ROWS_MAX));
        LH_HIP(ctx, hipMalloc((void**)&s->arg, 4 * SPEC_ROWS_MAX));
        LH_HIP(ctx, hipMalloc((void**)&s->win, 4 * ((size_t)m.ctx + 1)));
        if (p->attn_part) LH_HIP(ctx, hipMalloc((void**)&s->part, 4 * (size_t)SPEC_ROWS_MAX * m.H * ((m.ctx + ATT_TC - 1) / ATT_TC) * (m.hd + 2)));
    }
    int rc;
    if ((rc = grow(ctx, &s->corpus, &s->corpus_cap, n_corpus))) return rc;
    return grow(ctx, &s->trace, &s->trace_cap, n_trace, 2, 4096);
}
// the largest row count <= want a pass can take: 1 (the decode step) or a count of the bit-identical rows path
static uint32_t spec_pass_rows(const Plan* p, uint32_t want) {
    uint32_t n = std::min(want, gemv_rows_max(p->md.wtype));
    while (n > 1 && !rows_path_ok(p->ctx, p->md, n)) --n;
    return std::max(n, 1u);
}
// where the accept step's output list starts: the sampled loop's first id (the sample behind the prompt) is entry 0 of out_tokens_dev
static uint32_t* spec_out(const Plan* p) { return p->out_tokens_dev + (p->spec->smp ? 1 : 0); }
// the kernels of one pass of n rows, in stream order (n_table = rows of the table the accept step moves on)
static int spec_enqueue_pass(Plan* p, uint32_t n, uint32_t n_table, const SpecLookup& lp, int lookup_next) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& m = p->md;
    Spec* s = p->spec;
    int rc;
    if (n == 1) {   // the decode step's own kernels, token and position from the device
        if ((rc = enqueue_decode(p, s->sp, nullptr, nullptr, 0, nullptr))) return rc;
    } else {
        BatchCtx bc = {s->rows, s->tok, p->attn_part ? s->part : nullptr};
        if ((rc = plan_eval(p, nullptr, nullptr, nullptr, n, 0, false, &bc))) return rc;
    }
    if (s->smp) {
        if ((rc = sample_rows_launch(ctx, p->logits, m.V, n, p->ss_dev, p->ring_dev, s->tok, &s->st->k, s->arg, p->smp_topk))) return rc;
    } else {
        LH_LAUNCH(k_batch_argmax, dim3(n), dim3(1024), 0, ctx->stream, (const float*)p->logits, m.V, (BatchRow*)nullptr, (uint32_t*)nullptr, s->arg, (uint32_t*)nullptr, 0u,
                  (StepParams*)nullptr, 0);
    }
    LH_LAUNCH(k_spec_accept, dim3(1), dim3(SPEC_TH), 0, ctx->stream, (const uint32_t*)s->arg, n, s->st, s->rows, s->tok, s->sp, s->win, m.ctx, m.V, spec_out(p), s->trace,
              s->trace_cap, lp, n_table, lookup_next, s->smp ? p->ss_dev : (SampleState*)nullptr, s->smp ? p->ring_dev : (uint32_t*)nullptr);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// one full-width pass of the loop: eagerly the first time, then the captured graph (re-captured when a value it holds has changed)
static int spec_pass(Plan* p, uint32_t R, const SpecLookup& lp) {
    lh_ctx* ctx = p->ctx;
    Spec* s = p->spec;
    const Spec::Key key = {R, s->trace_cap, lp, spec_out(p), s->trace, ctx->splitk_gen, p->scratch_gen, s->smp, s->smp && p->smp_topk <= 64, s->smp ? p->ring_dev : nullptr, f16_stream_key(p)};
    f16_stream_sync(s->pass, &s->f16_seen, key.f16_stream);
    return s->pass.run(ctx, p->use_graph, R, key, " (speculative pass)", [&] { return spec_enqueue_pass(p, R, R, lp, 1); });
}
static int spec_set(Plan* p, uint32_t pos, uint32_t produced, uint32_t n_steps, const SpecToks& toks, uint32_t k, uint32_t n_rows, int reset) {
    lh_ctx* ctx = p->ctx;
    Spec* s = p->spec;
    LH_LAUNCH(k_spec_set, dim3(1), dim3(64), 0, ctx->stream, s->st, s->rows, s->tok, s->sp, p->md.kc, p->md.vc, pos, produced, n_steps, toks, k, n_rows, p->md.ctx, reset);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// window entries [0, pos) from the context's history and the pending token behind them, to the device
static int spec_upload_window(Plan* p, uint32_t pos, uint32_t pending) {
    lh_ctx* ctx = p->ctx;
    int rc;
    if ((rc = ensure_staging(ctx, ((uint64_t)pos + 1) * 4))) return rc;
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging reuse
    uint32_t* h = (uint32_t*)ctx->staging;
    for (uint32_t i = 0; i < pos; ++i) h[i] = (p->hist && i < p->hist->size()) ? (*p->hist)[i] : Plan::HIST_UNKNOWN;
    h[pos] = pending;
    LH_HIP(ctx, hipMemcpyAsync(p->spec->win, h, ((size_t)pos + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
static int spec_check_params(lh_ctx* ctx, const ModelDesc& md, const lh_lookup_params* lp, const char* who) {
    if (!lp) LH_FAIL(ctx, LH_EINVAL, "%s: no lookup parameters", who);
    const uint32_t kmax = gemv_rows_max(md.wtype) - 1;
    if (lp->draft_max < 1 || lp->draft_max > kmax) LH_FAIL(ctx, LH_EINVAL, "%s: draft_max %u (1..%u for this weight type)", who, lp->draft_max, kmax);
    if (lp->ngram_min < 1 || lp->ngram_min > lp->ngram_max || lp->ngram_max > SPEC_NGRAM_MAX)
        LH_FAIL(ctx, LH_EINVAL, "%s: n-gram bounds %u..%u (1 <= ngram_min <= ngram_max <= %u)", who, lp->ngram_min, lp->ngram_max, SPEC_NGRAM_MAX);
    if (lp->n_corpus > SPEC_CORPUS_MAX) LH_FAIL(ctx, LH_EINVAL, "%s: a corpus of %u tokens (at most %u)", who, lp->n_corpus, SPEC_CORPUS_MAX);
    if (lp->n_corpus && lp->corpus)
        for (uint32_t i = 0; i < lp->n_corpus; ++i)
            if (lp->corpus[i] >= md.V) LH_FAIL(ctx, LH_EINVAL, "%s: corpus id %u at index %u outside the vocabulary of %u", who, lp->corpus[i], i, md.V);
    return 0;
}

// sampled: the passes sample (sampler state and ring = the plan's ss_dev / ring_dev, armed by the caller, whose first id is entry 0 of the device's
// output list); the n_steps ids land behind it and out_tokens, when given, receives these n_steps ids.
static int spec_decode_lookup(Plan* p, uint32_t first_token, uint32_t past, uint32_t n_steps, const lh_lookup_params* lpar, uint32_t R, uint32_t* out_tokens,
                              float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap, bool sampled = false) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& md = p->md;
    int rc;
    const uint32_t n_corpus = lpar->corpus ? lpar->n_corpus : 0;
    if ((rc = spec_ensure(p, n_corpus, n_steps))) return rc;
    if ((rc = plan_ensure_rows(p, R))) return rc;
    if ((rc = ensure_out_tokens(p, n_steps + (sampled ? 1 : 0)))) return rc;
    Spec* s = p->spec;
    s->smp = sampled;
    if (n_corpus) {
        if ((rc = ensure_staging(ctx, (uint64_t)n_corpus * 4))) return rc;
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging reuse
        memcpy(ctx->staging, lpar->corpus, (size_t)n_corpus * 4);
        LH_HIP(ctx, hipMemcpyAsync(s->corpus, ctx->staging, (size_t)n_corpus * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    const SpecLookup lp = {n_corpus ? s->corpus : nullptr, n_corpus, R - 1, lpar->ngram_max, lpar->ngram_min};
    uint32_t pos = past, produced = 0, seg_pos0 = past;
    SpecState hs = {};
    std::vector<uint32_t> got, refeed;
    // the tokens the passes since seg_pos0 evaluated (window entries [seg_pos0, pos)) go into the context's history; returns the pending one
    auto learn = [&](uint32_t* pending) -> int {
        got.resize((size_t)pos - seg_pos0 + 1);
        LH_HIP(ctx, hipMemcpyAsync(got.data(), s->win + seg_pos0, got.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = seg_pos0; i < pos; ++i) p->record(i, got[i - seg_pos0]);
        *pending = got[pos - seg_pos0];
        return 0;
    };
    // state, table and first draft of a run of passes that starts with `pending` at position pos
    auto start = [&](uint32_t pending, int reset) -> int {
        if ((rc = spec_upload_window(p, pos, pending))) return rc;
        SpecToks t;
        for (uint32_t r = 0; r < SPEC_ROWS_MAX; ++r) t.t[r] = pending;
        if ((rc = spec_set(p, pos, produced, n_steps, t, 0, R, reset))) return rc;
        LH_LAUNCH(k_draft_lookup, dim3(1), dim3(SPEC_TH), 0, ctx->stream, (const uint32_t*)s->win, 0u, lp, 0u, md.V, s->tok, (uint32_t*)nullptr, s->st, md.ctx, R);
        LH_HIP(ctx, hipGetLastError());
        seg_pos0 = pos;
        return 0;
    };
    if (past < md.ctx && (rc = start(first_token, 1))) return rc;
    bool started = past < md.ctx;
    uint32_t pending = first_token;
    while (produced < n_steps) {
        if (pos >= md.ctx) {   // the context swap of the resident loops (server.go:160-172, resident_steps_swapping)
            if (started && (rc = learn(&pending))) return rc;
            if (p->keep >= md.ctx) LH_FAIL(ctx, LH_EINVAL, "context swap: KeepCount %u leaves no room in a window of %u", p->keep, md.ctx);
            if (!swap_refeed_tokens(p, pos, pending, &refeed))
                LH_FAIL(ctx, LH_EINVAL, "context swap at position %u: the tokens of the window are not known to this context (evaluate the prompt through it first)", pos);
            if (!refeed.empty() && (rc = plan_eval(p, refeed.data(), nullptr, nullptr, (uint32_t)refeed.size(), p->keep, true))) return rc;
            pos = p->keep + (uint32_t)refeed.size();
            if ((rc = plan_ensure_rows(p, R))) return rc;
            if ((rc = start(pending, started ? 0 : 1))) return rc;
            started = true;
        }
        const uint32_t n = spec_pass_rows(p, std::min(R, md.ctx - pos));
        if (n == R) {
            // `produced` and `pos` are exact here; q passes move them on by q..q*R: as many as can neither pass n_steps nor leave the window run unseen
            const uint32_t q = std::max(1u, std::min((n_steps - produced) / R, (md.ctx - pos) / R));
            for (uint32_t j = 0; j < q; ++j) if ((rc = spec_pass(p, R, lp))) return rc;
        } else if ((rc = spec_enqueue_pass(p, n, R, lp, 1))) {
            return rc;
        }
        LH_HIP(ctx, hipMemcpyAsync(&hs, s->st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (hs.produced <= produced) LH_FAIL(ctx, LH_EHIP, "lh_llama_decode_lookup: a pass produced no id");
        pos = hs.pos; produced = hs.produced;
    }
    if ((rc = learn(&pending))) return rc;
    if (out_tokens) LH_HIP(ctx, hipMemcpyAsync(out_tokens, spec_out(p), (size_t)n_steps * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (logits_last_host) LH_HIP(ctx, hipMemcpyAsync(logits_last_host, p->logits + (size_t)hs.last_a * md.V, (size_t)md.V * 4, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint16_t> tr;
    const uint32_t n_tr = trace ? std::min(std::min(trace_cap, hs.passes), s->trace_cap) : 0;
    if (n_tr) { tr.resize(n_tr); LH_HIP(ctx, hipMemcpyAsync(tr.data(), s->trace, (size_t)n_tr * 2, hipMemcpyDeviceToHost, ctx->stream)); }
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_tr) memcpy(trace, tr.data(), (size_t)n_tr * 2);
    if (stats) { stats->passes = hs.passes; stats->rows = R; stats->drafted = hs.drafted; stats->accepted = hs.accepted; stats->empty = hs.empty; }
    return 0;
}

// ---- lh_llama_decode_draft: a second model drafts (the rule is stated in include/llamahip.h) ------------------------------------------
// A pass of n rows = k_draft_model_begin (the draft's step parameters, st->k, filler), n one-token steps of the DRAFT plan - the decode step's own
// kernels, each step's greedy id written straight into the target's tok[j + 1] (the last step is there for the draft's cache row only) - then the
// target's pass over tok[0..n) exactly as the lookup loop runs it: plan_eval over the row table, k_batch_argmax, k_spec_accept with no next draft.
// State, table and tokens are the target's Spec; both plans sit on one lh_ctx, so one stream orders everything.  Every pass is enqueued kernel by
// kernel: the pass as ONE captured graph over both plans is left out (DESIGN 3i says why), so the launches of a pass are not replayed.
static int draft_enqueue_pass(Plan* p, Plan* d, uint32_t n, uint32_t n_table, uint32_t ctxw) {
    lh_ctx* ctx = p->ctx;
    Spec* s = p->spec;
    int rc;
    LH_TRACE("k_draft_model_begin/r%u", n);
    LH_LAUNCH(k_draft_model_begin, dim3(1), dim3(64), 0, ctx->stream, s->st, s->tok, d->sp_dev, n, n_table, ctxw);
    LH_HIP(ctx, hipGetLastError());
    for (uint32_t j = 0; j < n; ++j)
        if ((rc = enqueue_decode(d, d->sp_dev, nullptr, nullptr, 1, j + 1 < n ? s->tok + j + 1 : nullptr))) return rc;
    const SpecLookup none = {nullptr, 0, 0, 1, 1};
    return spec_enqueue_pass(p, n, n_table, none, 0);
}
static int spec_decode_draft(Plan* p, Plan* d, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t R, uint32_t* out_tokens, float* logits_last_host,
                             lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    lh_ctx* ctx = p->ctx;
    const ModelDesc& md = p->md;
    const uint32_t ctxw = std::min(md.ctx, d->md.ctx);
    int rc;
    // every allocation of both plans, in front of the first pass
    if ((rc = spec_ensure(p, 0, n_steps))) return rc;
    if ((rc = plan_ensure_rows(p, R))) return rc;
    if ((rc = ensure_out_tokens(p, n_steps))) return rc;
    if ((rc = ensure_out_tokens(d, SPEC_ROWS_MAX))) return rc;
    Spec* s = p->spec;
    s->smp = false;
    SpecToks t;
    for (uint32_t r = 0; r < SPEC_ROWS_MAX; ++r) t.t[r] = first_token;
    if ((rc = spec_set(p, past, 0, n_steps, t, 0, R, 1))) return rc;
    uint32_t pos = past, produced = 0;
    SpecState hs = {};
    while (produced < n_steps) {
        // past + n_steps <= ctxw (checked by the caller) and pos = past + produced: a position is left in both windows
        const uint32_t n = spec_pass_rows(p, std::min(R, ctxw - pos));
        if (n == R) {
            // `produced` and `pos` are exact here; q passes move them on by q..q*R: as many as can neither pass n_steps nor leave the window run unseen
            const uint32_t q = std::max(1u, std::min((n_steps - produced) / R, (ctxw - pos) / R));
            for (uint32_t j = 0; j < q; ++j) if ((rc = draft_enqueue_pass(p, d, R, R, ctxw))) return rc;
        } else if ((rc = draft_enqueue_pass(p, d, n, R, ctxw))) {   // the window's end: a narrower pass
            return rc;
        }
        LH_HIP(ctx, hipMemcpyAsync(&hs, s->st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (hs.produced <= produced || hs.produced > n_steps || hs.pos != past + hs.produced) LH_FAIL(ctx, LH_EHIP, "lh_llama_decode_draft: a pass left an inconsistent state");
        pos = hs.pos; produced = hs.produced;
    }
    std::vector<uint32_t> ids(n_steps);
    LH_HIP(ctx, hipMemcpyAsync(ids.data(), spec_out(p), (size_t)n_steps * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (logits_last_host) LH_HIP(ctx, hipMemcpyAsync(logits_last_host, p->logits + (size_t)hs.last_a * md.V, (size_t)md.V * 4, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint16_t> tr;
    const uint32_t n_tr = trace ? std::min(std::min(trace_cap, hs.passes), s->trace_cap) : 0;
    if (n_tr) { tr.resize(n_tr); LH_HIP(ctx, hipMemcpyAsync(tr.data(), s->trace, (size_t)n_tr * 2, hipMemcpyDeviceToHost, ctx->stream)); }
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // step i evaluated (i == 0 ? first_token : id i - 1) at position past + i, on both caches
    for (uint32_t i = 0; i < n_steps; ++i) {
        const uint32_t tk = i ? ids[i - 1] : first_token;
        p->record(past + i, tk);
        d->record(past + i, tk);
    }
    if (out_tokens) memcpy(out_tokens, ids.data(), (size_t)n_steps * 4);
    if (n_tr) memcpy(trace, tr.data(), (size_t)n_tr * 2);
    if (stats) { stats->passes = hs.passes; stats->rows = R; stats->drafted = hs.drafted; stats->accepted = hs.accepted; stats->empty = hs.empty; }
    return 0;
}

// ---- lh_batch_decode_lookup: the same loop for the pods of a batch -------------------------------------------------------------------
// A pass = the batched plan_eval of P * R rows on pod 0's plan (row i * R + r = row r of pod i, on pod i's cache: the table lh_batch_feed lays out for
// P pods fed R tokens each, with the per-row attention kernels), k_batch_argmax over the P * R logits rows, k_spec_accept_pods.  One captured graph.
// lh_batch_decode_sample_lookup (smp) exchanges two launches: k_sample_pod_rows / k_sample_small_pod_rows on the batch's sampler states and rings instead of
// k_batch_argmax, and the accept step commits every pod's ring and draw counter (ss_dev / ring_dev).
struct BatchSpec {
    SpecState* st = nullptr;           // [B]
    SpecPodSum* sum = nullptr;         // [B]
    BatchRow* rows = nullptr;          // [BATCH_ROWS_MAX]
    uint32_t* tok = nullptr;           // [BATCH_ROWS_MAX]
    uint32_t* arg = nullptr;           // [BATCH_ROWS_MAX]
    uint32_t* win = nullptr;           // [B][ctx + 1]
    float* last = nullptr;             // [B][V]
    float* part = nullptr;             // split-T attention partials for BATCH_ROWS_MAX rows (plans with ctx > 256)
    uint32_t* corpus = nullptr;
    uint32_t corpus_cap = 0;
    uint16_t* trace = nullptr;         // [B][trace_cap]
    uint32_t trace_cap = 0;
    bool smp = false;                  // the running loop samples (lh_batch_decode_sample_lookup)
    // the captured pass (warm bit n - 1: a pass of n rows) and what it holds by value
    struct Key {
        uint32_t R, trace_cap;
        SpecLookup lp;
        uint16_t* trace;
        uint64_t splitk_gen, scratch_gen;
        uint32_t smp, small_k;         // a sampled pass also holds the sampler variant, the state pointer, the ring pointer and its stride (zeros in a greedy one)
        SampleState* ss;
        uint32_t* ring;
        uint64_t ring_cap;
        uint64_t f16_stream;           // f16_stream_key
    };
    CapturedGraph<Key> pass;
    uint64_t f16_seen = 0;
};
static void batch_spec_free(Batch* b) {
    BatchSpec* s = b->spec;
    if (!s) return;
    s->pass.drop();
    void* bufs[] = {s->st, s->sum, s->rows, s->tok, s->arg, s->win, s->last, s->part, s->corpus, s->trace};
    for (void* q : bufs) if (q) hipFree(q);
    delete s;
    b->spec = nullptr;
}
// every allocation of the route, outside any capture
static int batch_spec_ensure(Batch* b, uint32_t n_corpus, uint32_t n_trace) {
    lh_ctx* ctx = b->ctx;
    Plan* p0 = b->pods[0];
    const ModelDesc& m = p0->md;
    const uint32_t B = b->B;
    if (!b->spec) b->spec = new BatchSpec();
    BatchSpec* s = b->spec;
    if (!s->st) {
        LH_HIP(ctx, hipMalloc((void**)&s->st, sizeof(SpecState) * B));
        LH_HIP(ctx, hipMalloc((void**)&s->sum, sizeof(SpecPodSum) * B));
        LH_HIP(ctx, hipMalloc((void**)&s->rows, sizeof(BatchRow) * BATCH_ROWS_MAX));
        LH_HIP(ctx, hipMalloc((void**)&s->tok, 4 * (size_t)BATCH_ROWS_MAX));
        LH_HIP(ctx, hipMalloc((void**)&s->arg, 4 * (size_t)BATCH_ROWS_MAX));
        LH_HIP(ctx, hipMalloc((void**)&s->win, 4 * (size_t)B * ((size_t)m.ctx + 1)));
        LH_HIP(ctx, hipMalloc((void**)&s->last, 4 * (size_t)B * m.V));
        if (p0->attn_part) LH_HIP(ctx, hipMalloc((void**)&s->part, 4 * (size_t)BATCH_ROWS_MAX * m.H * ((m.ctx + ATT_TC - 1) / ATT_TC) * (m.hd + 2)));
    }
    int rc;
    if ((rc = grow(ctx, &s->corpus, &s->corpus_cap, n_corpus))) return rc;
    return grow(ctx, &s->trace, &s->trace_cap, n_trace, 2 * (size_t)B, 256);   // (an element = one pass of every pod)
}
// rows per pod and pass: draft_max + 1, lowered to the largest R whose P * R rows share one weight pass on this plan; 1 = plain ticks.
// (A batch of one pod is never `batched` - one row needs no table - but its R rows are a batched Eval like any other.)
static uint32_t batch_spec_rows(const Batch* b, uint32_t draft_max) {
    if (!b->batched && b->B > 1) return 1;
    uint32_t R = draft_max + 1;
    while (R > 1 && (b->B * R > BATCH_ROWS_MAX || !plan_batch_rows_ok(b->pods[0], b->B * R))) --R;
    return R;
}
static SpecPodsArgs batch_spec_args(const Batch* b, uint32_t R) {
    const BatchSpec* s = b->spec;
    const ModelDesc& m = b->pods[0]->md;
    SpecPodsArgs a = {};
    a.arg = s->arg; a.st = s->st; a.rows = s->rows; a.tok = s->tok; a.win = s->win; a.out = b->out_dev; a.trace = s->trace;
    a.logits = b->pods[0]->logits; a.last = s->last; a.pend = b->tok_dev; a.ids = b->ids_dev; a.sum = s->sum;
    a.R = R; a.ctx = m.ctx; a.vocab = m.V; a.out_cap = b->out_cap; a.trace_cap = s->trace_cap;
    if (s->smp) { a.ss = b->ss_dev; a.ring = b->ring_dev; a.ring_cap = b->ring_cap; }
    return a;
}
// the kernels of one pass, in stream order
static int batch_spec_enqueue_pass(Batch* b, uint32_t R, const SpecLookup& lp) {
    lh_ctx* ctx = b->ctx;
    Plan* p0 = b->pods[0];
    const ModelDesc& m = p0->md;
    BatchSpec* s = b->spec;
    const uint32_t n = b->B * R;
    int rc;
    BatchCtx bc = {s->rows, s->tok, p0->attn_part ? s->part : nullptr};
    if ((rc = plan_eval(p0, nullptr, nullptr, nullptr, n, 0, false, &bc))) return rc;
    if (s->smp) {
        if ((rc = sample_pod_rows_launch(ctx, p0->logits, m.V, b->B, R, b->ss_dev, b->ring_dev, b->ring_cap, s->tok, s->st, s->arg, b->smp_topk))) return rc;
    } else {
        LH_LAUNCH(k_batch_argmax, dim3(n), dim3(1024), 0, ctx->stream, (const float*)p0->logits, m.V, (BatchRow*)nullptr, (uint32_t*)nullptr, s->arg, (uint32_t*)nullptr, 0u,
                  (StepParams*)nullptr, 0);
    }
    LH_LAUNCH(k_spec_accept_pods, dim3(b->B), dim3(SPEC_TH), 0, ctx->stream, batch_spec_args(b, R), lp, 1);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}
// one pass: eagerly the first time, then the captured graph (re-captured when a value it holds has changed)
static int batch_spec_pass(Batch* b, uint32_t R, const SpecLookup& lp) {
    lh_ctx* ctx = b->ctx;
    BatchSpec* s = b->spec;
    BatchSpec::Key key = {R, s->trace_cap, lp, s->trace, ctx->splitk_gen, b->scratch_gen(), s->smp, 0, nullptr, nullptr, 0, f16_stream_key(b->pods[0])};
    f16_stream_sync(s->pass, &s->f16_seen, key.f16_stream);
    if (s->smp) { key.small_k = b->smp_topk <= 64; key.ss = b->ss_dev; key.ring = b->ring_dev; key.ring_cap = b->ring_cap; }
    return s->pass.run(ctx, b->pods[0]->use_graph, b->B * R - 1, key, " (batch speculative pass)", [&] { return batch_spec_enqueue_pass(b, R, lp); });
}

// The loop behind lh_batch_decode_lookup and (smp) lh_batch_decode_sample_lookup; the caller has checked every argument and R >= 2.
static int batch_decode_lookup(Batch* b, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lpar, uint32_t R, uint32_t* out_tokens,
                               float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap, bool smp) {
    const char* who = smp ? "lh_batch_decode_sample_lookup" : "lh_batch_decode_lookup";
    lh_ctx* ctx = b->ctx;
    Plan* p0 = b->pods[0];
    const ModelDesc& m = p0->md;
    const uint32_t B = b->B, W = m.ctx + 1;
    int rc;
    const uint32_t n_corpus = lpar->corpus ? lpar->n_corpus : 0;
    // ---- every allocation first: none inside a capture
    if ((rc = batch_spec_ensure(b, n_corpus, n_steps))) return rc;
    if ((rc = plan_ensure_rows(p0, B * R))) return rc;   // (the captured tick re-captures on scratch_gen)
    const size_t win_bytes = 4 * (size_t)B * W;
    if ((rc = ensure_staging(ctx, win_bytes + 4 * (size_t)n_corpus))) return rc;
    BatchSpec* s = b->spec;
    s->smp = smp;
    // what the ticks so far did goes into the pods' histories (and waits for the stream: the staging buffer is free)
    if (b->pos_known) { if ((rc = batch_drain(b))) return rc; }
    else LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // ---- windows (positions [0, past_i) from the pod's history, the pending token behind them) and corpus: one upload each
    uint32_t* hw = (uint32_t*)ctx->staging;
    SpecPodsSet v = {};
    for (uint32_t i = 0; i < B; ++i) {
        const Plan* p = b->pods[i];
        uint32_t* h = hw + (size_t)i * W;
        for (uint32_t j = 0; j < W; ++j) h[j] = (j < past[i] && p->hist && j < p->hist->size()) ? (*p->hist)[j] : Plan::HIST_UNKNOWN;
        h[past[i]] = first_tokens[i];
        v.pos[i] = past[i]; v.tok[i] = first_tokens[i];
    }
    LH_HIP(ctx, hipMemcpyAsync(s->win, hw, win_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (n_corpus) {
        memcpy(ctx->staging + win_bytes, lpar->corpus, (size_t)n_corpus * 4);
        LH_HIP(ctx, hipMemcpyAsync(s->corpus, ctx->staging + win_bytes, (size_t)n_corpus * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    const SpecLookup lp = {n_corpus ? s->corpus : nullptr, n_corpus, R - 1, lpar->ngram_max, lpar->ngram_min};
    const SpecPodsArgs args = batch_spec_args(b, R);
    LH_LAUNCH(k_spec_set_pods, dim3(B), dim3(64), 0, ctx->stream, args, (const BatchRow*)b->rows_dev, v, n_steps);
    LH_LAUNCH(k_draft_lookup_pods, dim3(B), dim3(SPEC_TH), 0, ctx->stream, args, lp);
    LH_HIP(ctx, hipGetLastError());
    // ---- the passes.  Every pass gives every unfinished pod 1..R ids, so with `low` = the least count any pod has for certain, ceil((n_steps - low) / R)
    // passes cannot find every pod finished before the last of them; then one look at 16 bytes per pod.
    std::vector<SpecPodSum> hs(B);
    uint32_t low = 0;
    while (low < n_steps) {
        const uint32_t q = (n_steps - low + R - 1) / R;
        for (uint32_t j = 0; j < q; ++j) if ((rc = batch_spec_pass(b, R, lp))) return rc;
        LH_HIP(ctx, hipMemcpyAsync(hs.data(), s->sum, sizeof(SpecPodSum) * B, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        uint32_t now = n_steps;
        for (uint32_t i = 0; i < B; ++i) now = std::min(now, hs[i].produced);
        if (now < std::min(n_steps, low + q)) LH_FAIL(ctx, LH_EHIP, "%s: a pass produced no id for a pod", who);
        low = now;
    }
    // ---- results, then the state lh_batch_feed leaves: every pod behind its last evaluated token, its last id pending
    std::vector<uint32_t> out((size_t)B * n_steps);
    std::vector<SpecState> st(B);
    LH_HIP(ctx, hipMemcpy2DAsync(out.data(), (size_t)n_steps * 4, b->out_dev, (size_t)b->out_cap * 4, (size_t)n_steps * 4, B, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipMemcpyAsync(st.data(), s->st, sizeof(SpecState) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (logits_last_host) LH_HIP(ctx, hipMemcpyAsync(logits_last_host, s->last, 4 * (size_t)B * m.V, hipMemcpyDeviceToHost, ctx->stream));
    const uint32_t n_tr = trace ? std::min(std::min(trace_cap, n_steps), s->trace_cap) : 0;
    std::vector<uint16_t> tr((size_t)B * n_tr);
    if (n_tr) LH_HIP(ctx, hipMemcpy2DAsync(tr.data(), (size_t)n_tr * 2, s->trace, (size_t)s->trace_cap * 2, (size_t)n_tr * 2, B, hipMemcpyDeviceToHost, ctx->stream));
    LH_LAUNCH(k_batch_feed_heads, dim3(1), dim3(64), 0, ctx->stream, b->out_dev, b->out_cap, (const uint32_t*)b->tok_dev, B);
    LH_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> newpos(B);
    for (uint32_t i = 0; i < B; ++i) newpos[i] = past[i] + n_steps;
    if ((rc = batch_set(b, nullptr, newpos.data(), 1))) return rc;
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < B; ++i) {
        if (st[i].produced != n_steps || st[i].pos != newpos[i]) LH_FAIL(ctx, LH_EHIP, "%s: the accept step left pod %u in an inconsistent state", who, i);
        const uint32_t* o = out.data() + (size_t)i * n_steps;
        for (uint32_t t = 0; t < n_steps; ++t) b->pods[i]->record(past[i] + t, t ? o[t - 1] : first_tokens[i]);
        memcpy(out_tokens + (size_t)i * n_steps, o, (size_t)n_steps * 4);
        if (stats) stats[i] = lh_spec_stats{st[i].passes, R, st[i].drafted, st[i].accepted, st[i].empty};
        if (n_tr) {
            const uint32_t np = std::min(n_tr, st[i].passes);
            memcpy(trace + (size_t)i * trace_cap, tr.data() + (size_t)i * n_tr, (size_t)np * 2);
        }
    }
    return 0;
}

}  // namespace lh

using namespace lh;

// ======================================================================================================
// C-ABI
// ======================================================================================================
extern "C" {

void lh_ctx_destroy(lh_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    destroy_plans(ctx);
    if (ctx->arena) hipFree(ctx->arena);
    if (ctx->splitk) hipFree(ctx->splitk);
    if (ctx->xs3) hipFree(ctx->xs3);
    for (auto& w : ctx->wide) hipFree(w.second);
    if (ctx->tc_ev0) { hipEventDestroy(ctx->tc_ev0); hipEventDestroy(ctx->tc_ev1); }
    if (ctx->staging) hipHostFree(ctx->staging);
    if (ctx->out_pinned) hipHostFree(ctx->out_pinned);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

// The two greedy kernels on host logits (op-level parity, the twin of lh_sample_top_p_top_k / lh_score_rows).  Rows are packed: with
// n_logits % 4 != 0 the rows behind the first are not 16-byte aligned, which is what takes k_argmax_advance down its 4-byte path.
int lh_argmax_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_rows, uint32_t n_logits, int which, uint32_t* ids_out_host) {
    if (!ctx) return LH_EINVAL;
    if (!logits_host || !ids_out_host) LH_FAIL(ctx, LH_EINVAL, "lh_argmax_rows: null argument");
    if (n_logits == 0 || n_logits > 64u * 1024u) LH_FAIL(ctx, LH_ESHAPE, "lh_argmax_rows: vocabulary of %u ids outside the supported 1..65536", n_logits);
    if (n_rows == 0) LH_FAIL(ctx, LH_EINVAL, "lh_argmax_rows: no rows");
    if (which != 0 && which != 1) LH_FAIL(ctx, LH_EINVAL, "lh_argmax_rows: which = %d (0 = k_argmax_advance per row, 1 = k_batch_argmax)", which);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: logits | ids
    const size_t o_ids = (((size_t)n_rows * n_logits * 4) + 15) & ~(size_t)15, total = o_ids + (size_t)n_rows * 4;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    const float* lg = (const float*)dev;
    uint32_t* ids = (uint32_t*)(dev + o_ids);
    hipError_t e = hipMemcpyAsync(dev, logits_host, (size_t)n_rows * n_logits * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's array is pageable host memory
    if (e == hipSuccess) {
        if (which == 0) {
            for (uint32_t r = 0; r < n_rows; ++r)
                LH_LAUNCH(k_argmax_advance, dim3(1), dim3(1024), 0, ctx->stream, lg + (size_t)r * n_logits, n_logits, (StepParams*)nullptr, (uint32_t*)nullptr, ids + r, 0);
        } else {
            LH_LAUNCH(k_batch_argmax, dim3(n_rows), dim3(1024), 0, ctx->stream, lg, n_logits, (BatchRow*)nullptr, (uint32_t*)nullptr, ids, (uint32_t*)nullptr, 0u,
                      (StepParams*)nullptr, 0);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(ids_out_host, ids, (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_argmax_rows: %s", hipGetErrorString(e));
    return LH_OK;
}

int lh_llama_create(lh_ctx* ctx, const lh_llama_desc* desc, lh_llama** out) {
    if (!ctx || !desc || !out) LH_FAIL(ctx, LH_EINVAL, "lh_llama_create: NULL argument");
    *out = nullptr;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (desc->weight_dtype != 0 && desc->weight_dtype != 1 && desc->weight_dtype != 2 && desc->weight_dtype != 7) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_create: weight dtype %d not supported", desc->weight_dtype);
    ModelDesc md;
    md.V = desc->vocab; md.d = desc->embd; md.H = desc->heads; md.L = desc->layers; md.F = desc->ff; md.ctx = desc->ctx;
    if (!md.H || !md.d || md.d % md.H) LH_FAIL(ctx, LH_ESHAPE, "lh_llama_create: bad embd/heads");
    md.hd = md.d / md.H;
    md.layer0 = desc->layer0; md.layer1 = desc->layer1 ? desc->layer1 : desc->layers;
    if (md.layer0 >= md.layer1 || md.layer1 > md.L) LH_FAIL(ctx, LH_EINVAL, "lh_llama_create: bad layer range [%u,%u)", md.layer0, md.layer1);
    md.cache_layer0 = md.layer0;
    md.wtype = desc->weight_dtype;
    auto need = [&](lh_buf b, uint64_t n, const char* what, const float** dst) -> int {
        Buffer* bf = find_buffer(ctx->ds, b);
        if (!bf) LH_FAIL(ctx, LH_EINVAL, "lh_llama_create: %s is not a registered buffer", what);
        if (bf->nfloats < n) LH_FAIL(ctx, LH_ESHAPE, "lh_llama_create: %s has %llu floats, needs %llu", what, (unsigned long long)bf->nfloats, (unsigned long long)n);
        if (bf->dtype != 0) LH_FAIL(ctx, LH_ESHAPE, "lh_llama_create: %s must be f32", what);
        *dst = bf->dev;
        return 0;
    };
    // weight matrix: f32, or block-int8 planes when the model is quantised
    auto needw = [&](lh_buf b, uint64_t rows, uint64_t cols, const char* what, const float** dst, const float** sc) -> int {
        Buffer* bf = find_buffer(ctx->ds, b);
        if (!bf) LH_FAIL(ctx, LH_EINVAL, "lh_llama_create: %s is not a registered buffer", what);
        if (md.wtype == 1 && bf->dtype != 1) LH_FAIL(ctx, LH_EINVAL, "lh_llama_create: weight_dtype 1 (f16) but %s is a dtype-%d buffer: every matrix of an f16 model must be f16", what, bf->dtype);
        if (bf->nfloats < rows * cols || bf->dtype != md.wtype) LH_FAIL(ctx, LH_ESHAPE, "lh_llama_create: %s has the wrong size or dtype", what);
        if ((md.wtype == 7 || md.wtype == 2) && (bf->rows != rows || bf->cols != cols)) LH_FAIL(ctx, LH_ESHAPE, "lh_llama_create: %s %s shape mismatch", what, md.wtype == 7 ? "block-int8" : "block-int4");
        *dst = bf->dev;
        *sc = bf->scales;
        return 0;
    };
    int rc;
    const uint64_t d = md.d, F = md.F, V = md.V;
    if (md.first_stage() && (rc = need(desc->tok_embeddings, V * d, "tok_embeddings", &md.tok_emb))) return rc;
    if (md.last_stage()) {
        if ((rc = need(desc->norm, d, "norm", &md.norm))) return rc;
        if ((rc = needw(desc->output, V, d, "output", &md.output, &md.s_output))) return rc;
    }
    md.layers.resize(md.L);
    for (uint32_t il = md.layer0; il < md.layer1; ++il) {
        const lh_llama_layer& s = desc->layer[il];
        LayerW& L = md.layers[il];
        if ((rc = need(s.attention_norm, d, "attention_norm", &L.attn_norm))) return rc;
        if ((rc = needw(s.wq, d, d, "wq", &L.wq, &L.s_wq))) return rc;
        if ((rc = needw(s.wk, d, d, "wk", &L.wk, &L.s_wk))) return rc;
        if ((rc = needw(s.wv, d, d, "wv", &L.wv, &L.s_wv))) return rc;
        if ((rc = needw(s.wo, d, d, "wo", &L.wo, &L.s_wo))) return rc;
        if ((rc = need(s.ffn_norm, d, "ffn_norm", &L.ffn_norm))) return rc;
        if ((rc = needw(s.w1, F, d, "w1", &L.w1, &L.s_w1))) return rc;
        if ((rc = needw(s.w2, d, F, "w2", &L.w2, &L.s_w2))) return rc;
        if ((rc = needw(s.w3, F, d, "w3", &L.w3, &L.s_w3))) return rc;
    }
    const float *kc, *vc;
    const uint64_t kvn = d * (md.layer1 - md.layer0) * md.ctx;
    if ((rc = need(desc->k_cache, kvn, "k_cache", &kc))) return rc;
    if ((rc = need(desc->v_cache, kvn, "v_cache", &vc))) return rc;
    md.kc = (float*)kc; md.vc = (float*)vc;
    {   // the cache's token history travels with the buffer: shared with the graph path's plan over the same cache
        Buffer* kb = find_buffer(ctx->ds, desc->k_cache);
        if (!kb->kv_hist) kb->kv_hist = std::make_shared<std::vector<uint32_t>>();
        md.kv_hist = kb->kv_hist;
    }
    Plan* p = nullptr;
    if ((rc = plan_create(ctx, md, &p))) return rc;
    lh_llama* m = new lh_llama();
    m->ctx = ctx;
    m->plan = p;
    *out = m;
    return LH_OK;
}

void lh_llama_destroy(lh_llama* m) {
    if (!m) return;
    plan_destroy(m->plan);
    delete m;
}

int lh_llama_eval(lh_llama* m, const uint32_t* tokens, uint32_t n, uint32_t past, float* logits_host) {
    if (!m || !tokens) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!p->md.first_stage() || !p->md.last_stage()) LH_FAIL(ctx, LH_EINVAL, "lh_llama_eval needs a whole-model plan; use lh_llama_stage");
    int rc = plan_eval(p, tokens, nullptr, nullptr, n, past, true);
    if (rc) return rc;
    if (logits_host)
        LH_HIP(ctx, hipMemcpyAsync(logits_host, p->logits + (size_t)(n - 1) * p->md.V, (size_t)p->md.V * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

int lh_llama_set_keep(lh_llama* m, uint32_t keep) {
    if (!m) return LH_EINVAL;
    m->plan->keep = keep;
    return LH_OK;
}

int lh_llama_decode_greedy(lh_llama* m, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t* out_tokens, float* logits_last_host) {
    if (!m || !n_steps) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!md.first_stage() || !md.last_stage()) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_greedy needs a whole-model plan");
    if (past > md.ctx) LH_FAIL(ctx, LH_EINVAL, "decode: position %u outside the context window of %u", past, md.ctx);
    if (first_token >= md.V) LH_FAIL(ctx, LH_EINVAL, "decode: token id %u outside the vocabulary of %u", first_token, md.V);
    int rc;
    if ((rc = ensure_out_tokens(p, n_steps))) return rc;
    if ((rc = upload_step_params(p, 0, first_token, past, 0))) return rc;
    // past + n_steps > ctx: the loop swaps context like server.Do does (server.go:160-172) instead of failing
    if ((rc = resident_steps_swapping(p, first_token, &past, 0, n_steps, false))) return rc;
    if (out_tokens) LH_HIP(ctx, hipMemcpyAsync(out_tokens, p->out_tokens_dev, (size_t)n_steps * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (logits_last_host) LH_HIP(ctx, hipMemcpyAsync(logits_last_host, p->logits, (size_t)md.V * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

int lh_draft_lookup(lh_ctx* ctx, const uint32_t* window, uint32_t n_window, const lh_lookup_params* lp, uint32_t limit, uint32_t* draft_out, uint32_t* n_draft) {
    if (!ctx) return LH_EINVAL;
    if (!window || !n_window || !lp || !draft_out || !n_draft) LH_FAIL(ctx, LH_EINVAL, "lh_draft_lookup: null argument or empty window");
    if (lp->draft_max < 1 || lp->draft_max > SPEC_ROWS_MAX - 1) LH_FAIL(ctx, LH_EINVAL, "lh_draft_lookup: draft_max %u (1..%u)", lp->draft_max, SPEC_ROWS_MAX - 1);
    if (lp->ngram_min < 1 || lp->ngram_min > lp->ngram_max || lp->ngram_max > SPEC_NGRAM_MAX)
        LH_FAIL(ctx, LH_EINVAL, "lh_draft_lookup: n-gram bounds %u..%u (1 <= ngram_min <= ngram_max <= %u)", lp->ngram_min, lp->ngram_max, SPEC_NGRAM_MAX);
    if (lp->n_corpus > SPEC_CORPUS_MAX) LH_FAIL(ctx, LH_EINVAL, "lh_draft_lookup: a corpus of %u tokens (at most %u)", lp->n_corpus, SPEC_CORPUS_MAX);
    if (n_window > (1u << 24)) LH_FAIL(ctx, LH_EINVAL, "lh_draft_lookup: a window of %u tokens", n_window);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t nc = lp->corpus ? lp->n_corpus : 0;
    // one allocation: window | corpus | draft | count
    const size_t o_c = (size_t)n_window * 4, o_d = o_c + (size_t)nc * 4, o_k = o_d + 4 * SPEC_ROWS_MAX, total = o_k + 4;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    uint32_t res[SPEC_ROWS_MAX + 1] = {};
    hipError_t e = hipMemcpyAsync(dev, window, o_c, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && nc) e = hipMemcpyAsync(dev + o_c, lp->corpus, (size_t)nc * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's arrays are pageable host memory
    if (e == hipSuccess) {
        const SpecLookup dl = {nc ? (const uint32_t*)(dev + o_c) : nullptr, nc, lp->draft_max, lp->ngram_max, lp->ngram_min};
        LH_LAUNCH(k_draft_lookup, dim3(1), dim3(SPEC_TH), 0, ctx->stream, (const uint32_t*)dev, n_window, dl, limit, SPEC_UNKNOWN, (uint32_t*)(dev + o_d), (uint32_t*)(dev + o_k),
                  (SpecState*)nullptr, 0u, 0u);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(res, dev + o_d, sizeof res, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_draft_lookup: %s", hipGetErrorString(e));
    *n_draft = res[SPEC_ROWS_MAX];
    for (uint32_t i = 0; i < res[SPEC_ROWS_MAX] && i < lp->draft_max; ++i) draft_out[i] = res[i];
    return LH_OK;
}

int lh_llama_verify(lh_llama* m, const uint32_t* tokens, uint32_t n, uint32_t past, uint32_t* ids_out, uint32_t* n_accepted, float* logits_host) {
    if (!m) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    if (!tokens || !ids_out || !n_accepted) LH_FAIL(ctx, LH_EINVAL, "lh_llama_verify: null argument");
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!md.first_stage() || !md.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_verify needs a whole-model plan (layers [%u, %u) of %u)", md.layer0, md.layer1, md.L);
    if (n < 1 || n > gemv_rows_max(md.wtype)) LH_FAIL(ctx, LH_EINVAL, "lh_llama_verify: %u rows (1..%u for this weight type)", n, gemv_rows_max(md.wtype));
    if ((uint64_t)past + n > md.ctx) LH_FAIL(ctx, LH_EINVAL, "lh_llama_verify: past %u + n %u exceeds the context window of %u", past, n, md.ctx);
    for (uint32_t i = 0; i < n; ++i)
        if (tokens[i] >= md.V) LH_FAIL(ctx, LH_EINVAL, "lh_llama_verify: token id %u at index %u outside the vocabulary of %u", tokens[i], i, md.V);
    if (n > 1 && !rows_path_ok(ctx, md, n)) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_verify: this model's shapes have no %u-row pass on the decode stream", n);
    int rc;
    if ((rc = spec_ensure(p, 0, n))) return rc;
    if ((rc = plan_ensure_rows(p, n))) return rc;
    if ((rc = ensure_out_tokens(p, n))) return rc;
    Spec* s = p->spec;
    s->smp = false;
    SpecToks t = {};
    for (uint32_t i = 0; i < SPEC_ROWS_MAX; ++i) t.t[i] = tokens[i < n ? i : 0];
    if ((rc = spec_set(p, past, 0, n, t, n - 1, n, 1))) return rc;
    const SpecLookup none = {nullptr, 0, 0, 1, 1};
    if ((rc = spec_enqueue_pass(p, n, n, none, 0))) return rc;
    SpecState hs = {};
    uint32_t ids[SPEC_ROWS_MAX] = {};
    LH_HIP(ctx, hipMemcpyAsync(&hs, s->st, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipMemcpyAsync(ids, p->out_tokens_dev, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t a = hs.last_a;
    if (hs.produced != a + 1 || a >= n) LH_FAIL(ctx, LH_EHIP, "lh_llama_verify: the accept step left an inconsistent state");
    if (logits_host) {
        LH_HIP(ctx, hipMemcpyAsync(logits_host, p->logits + (size_t)a * md.V, (size_t)md.V * 4, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (uint32_t i = 0; i <= a; ++i) { p->record(past + i, tokens[i]); ids_out[i] = ids[i]; }
    *n_accepted = a;
    return LH_OK;
}

int lh_llama_decode_lookup(lh_llama* m, uint32_t first_token, uint32_t past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out_tokens, float* logits_last_host,
                           lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    if (!m || !n_steps) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!md.first_stage() || !md.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_decode_lookup needs a whole-model plan (layers [%u, %u) of %u)", md.layer0, md.layer1, md.L);
    int rc;
    if ((rc = spec_check_params(ctx, md, lp, "lh_llama_decode_lookup"))) return rc;
    if (past > md.ctx) LH_FAIL(ctx, LH_EINVAL, "decode: position %u outside the context window of %u", past, md.ctx);
    if (first_token >= md.V) LH_FAIL(ctx, LH_EINVAL, "decode: token id %u outside the vocabulary of %u", first_token, md.V);
    const uint32_t R = spec_pass_rows(p, lp->draft_max + 1);
    if (R == 1) {   // no multi-row pass on this plan's shapes: plain greedy steps, and the stats say so
        if ((rc = lh_llama_decode_greedy(m, first_token, past, n_steps, out_tokens, logits_last_host))) return rc;
        if (stats) { stats->passes = n_steps; stats->rows = 1; stats->drafted = 0; stats->accepted = 0; stats->empty = n_steps; }
        if (trace) for (uint32_t i = 0; i < n_steps && i < trace_cap; ++i) trace[i] = 0;
        return LH_OK;
    }
    return spec_decode_lookup(p, first_token, past, n_steps, lp, R, out_tokens, logits_last_host, stats, trace, trace_cap);
}

int lh_llama_decode_draft(lh_llama* target, lh_llama* draft, uint32_t first_token, uint32_t past, uint32_t n_steps, uint32_t draft_len, uint32_t* out_tokens,
                          float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    if (!target || !draft) return LH_EINVAL;
    lh_ctx* ctx = target->ctx;
    Plan* p = target->plan;
    Plan* d = draft->plan;
    if (!n_steps) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: n_steps = 0");
    const ModelDesc& md = p->md;
    const ModelDesc& dd = d->md;
    if (draft == target || d == p) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: the draft is the target itself (a draft needs a cache of its own)");
    if (draft->ctx != ctx) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: target and draft belong to different lh_ctx (one stream must order both)");
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!md.first_stage() || !md.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_decode_draft: the target needs a whole-model plan (layers [%u, %u) of %u)", md.layer0, md.layer1, md.L);
    if (!dd.first_stage() || !dd.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_decode_draft: the draft needs a whole-model plan (layers [%u, %u) of %u)", dd.layer0, dd.layer1, dd.L);
    if (dd.V != md.V) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: vocabularies differ (target %u, draft %u)", md.V, dd.V);
    const uint32_t kmax = gemv_rows_max(md.wtype) - 1;
    if (draft_len < 1 || draft_len > kmax) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: draft_len %u (1..%u for the target's weight type)", draft_len, kmax);
    if (first_token >= md.V) LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: token id %u outside the vocabulary of %u", first_token, md.V);
    const uint32_t ctxw = std::min(md.ctx, dd.ctx);
    if ((uint64_t)past + n_steps > ctxw)
        LH_FAIL(ctx, LH_EINVAL, "lh_llama_decode_draft: past %u + n_steps %u exceeds the context window of %u (the smaller of target %u and draft %u; this loop does not swap context)",
                past, n_steps, ctxw, md.ctx, dd.ctx);
    int rc;
    const uint32_t R = spec_pass_rows(p, draft_len + 1);
    if (R == 1) {   // no multi-row pass on the target's shapes: plain greedy steps of the target, nothing is drafted
        std::vector<uint32_t> ids(n_steps);
        if ((rc = lh_llama_decode_greedy(target, first_token, past, n_steps, ids.data(), logits_last_host))) return rc;
        // the draft's cache and history follow in ONE Eval of the tokens the steps evaluated, so that the state both contexts are left in does not depend on R
        std::vector<uint32_t> ev(n_steps);
        for (uint32_t i = 0; i < n_steps; ++i) ev[i] = i ? ids[i - 1] : first_token;
        if ((rc = plan_eval(d, ev.data(), nullptr, nullptr, n_steps, past, true))) return rc;
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (out_tokens) memcpy(out_tokens, ids.data(), (size_t)n_steps * 4);
        if (stats) { stats->passes = n_steps; stats->rows = 1; stats->drafted = 0; stats->accepted = 0; stats->empty = n_steps; }
        if (trace) for (uint32_t i = 0; i < n_steps && i < trace_cap; ++i) trace[i] = 0;
        return LH_OK;
    }
    return spec_decode_draft(p, d, first_token, past, n_steps, R, out_tokens, logits_last_host, stats, trace, trace_cap);
}

}  // extern "C"

// lh_llama_decode_sample (lp == nullptr) and lh_llama_decode_sample_lookup (lp: checked by the caller, R >= 2 rows per pass): the same ring, prompt
// Eval and first sample; the n_predict - 1 ids behind it by resident steps, or by verify passes that sample every row.
static int decode_sample(lh_llama* m, const char* who, const uint32_t* prompt, uint32_t n_prompt, uint32_t n_predict, uint32_t ring_size, const lh_sample_params* sp,
                         uint32_t* out_tokens, const lh_lookup_params* lp, uint32_t R, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    if (!prompt || !n_prompt || !n_predict || !out_tokens) LH_FAIL(ctx, LH_EINVAL, "%s: empty prompt, no tokens to predict or null output", who);
    if (!md.first_stage() || !md.last_stage()) LH_FAIL(ctx, LH_EINVAL, "%s needs a whole-model plan", who);
    if (ring_size == 0) LH_FAIL(ctx, LH_EINVAL, "%s: the lastNTokens ring needs at least one slot (the reference uses CtxSize, server.go:127)", who);
    if (n_prompt > md.ctx) LH_FAIL(ctx, LH_EINVAL, "decode: a prompt of %u tokens exceeds the context window of %u", n_prompt, md.ctx);
    int rc;
    if ((rc = sample_check(ctx, sp, md.V))) return rc;
    if ((rc = ensure_out_tokens(p, n_predict))) return rc;
    if (!p->ss_dev) LH_HIP(ctx, hipMalloc((void**)&p->ss_dev, sizeof(SampleState)));
    if ((sp->top_k <= 64) != (p->smp_topk <= 64)) p->smp_gen++;  // the captured sampled steps hold the kernel variant
    p->smp_topk = sp->top_k;
    if ((rc = grow(ctx, &p->ring_dev, &p->ring_cap, ring_size, 4, 0, &p->smp_gen))) return rc;  // ... and the ring pointer
    // ring: ring_size zeros, then the prompt ids (appendToken, server.go:129-138, 193-197): what remains is the last ring_size of them
    {
        std::vector<uint32_t> ring(ring_size, 0u);
        for (uint32_t i = 0; i < n_prompt; ++i) ring[i % ring_size] = prompt[i];
        SampleState st = {sp->top_k, sp->top_p, sp->temp, sp->repeat_penalty, sp->seed, 0, ring_size, n_prompt};
        if ((rc = ensure_staging(ctx, (uint64_t)ring_size * 4 + sizeof st))) return rc;
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging reuse
        memcpy(ctx->staging, ring.data(), (size_t)ring_size * 4);
        memcpy((char*)ctx->staging + (size_t)ring_size * 4, &st, sizeof st);
        LH_HIP(ctx, hipMemcpyAsync(p->ring_dev, ctx->staging, (size_t)ring_size * 4, hipMemcpyHostToDevice, ctx->stream));
        LH_HIP(ctx, hipMemcpyAsync(p->ss_dev, (char*)ctx->staging + (size_t)ring_size * 4, sizeof st, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = plan_eval(p, prompt, nullptr, nullptr, n_prompt, 0, true))) return rc;
    // first sample on the last prompt row; the bookkeeping moves {past: n_prompt - 1, step: 0} to {token, past: n_prompt, step: 1}
    if ((rc = upload_step_params(p, 0, 0, n_prompt - 1, 0))) return rc;
    const float* last_row = n_prompt == 1 ? p->logits : p->logits + (size_t)(n_prompt - 1) * md.V;
    if ((rc = sample_launch(ctx, last_row, md.V, p->ss_dev, p->ring_dev, p->sp_dev, p->out_tokens_dev, nullptr, nullptr, nullptr, nullptr, 1, p->smp_topk))) return rc;
    if (n_predict > 1 && lp) {
        // the passes need the pending token on the host (window upload, first draft): one look per generation, then the loop of spec_decode_lookup
        // with this plan's sampler state; its ids land behind the first one
        uint32_t first = 0;
        LH_HIP(ctx, hipMemcpyAsync(&first, p->out_tokens_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = spec_decode_lookup(p, first, n_prompt, n_predict - 1, lp, R, nullptr, nullptr, stats, trace, trace_cap, /*sampled=*/true))) return rc;
    } else if (n_predict > 1) {
        // the first id (entry 0 of the output list) is the first token the resident steps evaluate; past the window the loop swaps context
        // (server.go:160-172)
        uint32_t past = n_prompt;
        if ((rc = resident_steps_swapping(p, 0, &past, 1, n_predict - 1, true, /*first_in_out=*/true))) return rc;
    } else if (lp && stats) {
        *stats = lh_spec_stats{0, R, 0, 0, 0};
    }
    LH_HIP(ctx, hipMemcpyAsync(out_tokens, p->out_tokens_dev, (size_t)n_predict * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

extern "C" {

int lh_llama_decode_sample(lh_llama* m, const uint32_t* prompt, uint32_t n_prompt, uint32_t n_predict, uint32_t ring_size, const lh_sample_params* sp,
                           uint32_t* out_tokens) {
    if (!m) return LH_EINVAL;
    LH_HIP(m->ctx, hipSetDevice(m->ctx->device));
    return decode_sample(m, "lh_llama_decode_sample", prompt, n_prompt, n_predict, ring_size, sp, out_tokens, nullptr, 1, nullptr, nullptr, 0);
}

int lh_llama_decode_sample_lookup(lh_llama* m, const uint32_t* prompt, uint32_t n_prompt, uint32_t n_predict, uint32_t ring_size, const lh_sample_params* sp,
                                  const lh_lookup_params* lp, uint32_t* out_tokens, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    if (!m) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!md.first_stage() || !md.last_stage())
        LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_decode_sample_lookup needs a whole-model plan (layers [%u, %u) of %u)", md.layer0, md.layer1, md.L);
    int rc;
    if ((rc = spec_check_params(ctx, md, lp, "lh_llama_decode_sample_lookup"))) return rc;
    const uint32_t R = spec_pass_rows(p, lp->draft_max + 1);
    if (R == 1) {   // no multi-row pass on this plan's shapes: plain sampled steps, and the stats say so
        if ((rc = decode_sample(m, "lh_llama_decode_sample_lookup", prompt, n_prompt, n_predict, ring_size, sp, out_tokens, nullptr, 1, nullptr, nullptr, 0))) return rc;
        const uint32_t n = n_predict - 1;
        if (stats) *stats = lh_spec_stats{n, 1, 0, 0, n};
        if (trace) for (uint32_t i = 0; i < n && i < trace_cap; ++i) trace[i] = 0;
        return LH_OK;
    }
    return decode_sample(m, "lh_llama_decode_sample_lookup", prompt, n_prompt, n_predict, ring_size, sp, out_tokens, lp, R, stats, trace, trace_cap);
}

int lh_llama_stage(lh_llama* m, const uint32_t* tokens, const uint32_t* tokens_dev, const float* x_in_dev, float* x_out_dev, uint32_t n, uint32_t past,
                   float* logits_dev, uint32_t* argmax_dev) {
    if (!m) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if (n == 1) {
        if ((rc = plan_ensure_rows(p, 1))) return rc;
        if ((uint64_t)past + 1 > md.ctx) LH_FAIL(ctx, LH_EINVAL, "stage: position %u outside the context window", past);
        const uint32_t slot = 1 + (p->slot_counter++ % (SP_SLOTS - 1));
        if (md.first_stage() && !tokens && !tokens_dev) LH_FAIL(ctx, LH_EINVAL, "stage: first stage needs a token id (host or device)");
        if (md.first_stage() && tokens && tokens[0] >= md.V) LH_FAIL(ctx, LH_EINVAL, "stage: token id %u outside the vocabulary of %u", tokens[0], md.V);
        if (past < p->share_len) p->share_broken = true;   // (this path records no token: the note of Plan::record, made here)
        if ((rc = upload_step_params(p, slot, tokens ? tokens[0] : 0, past, 0))) return rc;
        if ((rc = enqueue_decode(p, p->sp_dev + slot, x_in_dev, x_out_dev, false, md.last_stage() ? argmax_dev : nullptr, tokens ? nullptr : tokens_dev))) return rc;
    } else {
        if (md.first_stage() && !tokens) LH_FAIL(ctx, LH_EINVAL, "stage: multi-row first stage needs host token ids");
        if ((rc = plan_eval(p, tokens, x_in_dev, x_out_dev, n, past, true))) return rc;
        if (md.last_stage() && argmax_dev) {
            LH_LAUNCH(k_argmax_advance, dim3(1), dim3(1024), 0, ctx->stream, (const float*)(p->logits + (size_t)(n - 1) * md.V), md.V, (StepParams*)nullptr,
                               (uint32_t*)nullptr, argmax_dev, 0);
            LH_HIP(ctx, hipGetLastError());
        }
    }
    if (md.last_stage() && logits_dev)
        LH_HIP(ctx, hipMemcpyAsync(logits_dev, p->logits + (size_t)(n - 1) * md.V, (size_t)md.V * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return LH_OK;
}

// ---- lh_batch ---------------------------------------------------------------------------------------------------------------------
struct lh_batch { lh::Batch* b; };

int lh_batch_create(lh_ctx* ctx, lh_llama* const* pods, uint32_t n_pods, lh_batch** out) {
    if (!ctx || !pods || !out) LH_FAIL(ctx, LH_EINVAL, "lh_batch_create: NULL argument");
    *out = nullptr;
    if (n_pods == 0 || n_pods > 64) LH_FAIL(ctx, LH_EINVAL, "lh_batch_create: %u rows outside 1..64", n_pods);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    Batch* b = new Batch();
    b->ctx = ctx;
    b->B = n_pods;
    for (uint32_t i = 0; i < n_pods; ++i) {
        if (!pods[i] || pods[i]->ctx != ctx) { delete b; LH_FAIL(ctx, LH_EINVAL, "lh_batch_create: pod %u lives on another context (one stream orders the tick)", i); }
        Plan* p = pods[i]->plan;
        if (i > 0) {
            // same weights, same layer range, same shape; only the KV cache differs (a llama.Context per pod over one Model, server.go:151)
            ModelDesc a = p->md, c = b->pods[0]->md;
            a.kc = c.kc; a.vc = c.vc;
            if (!a.same(c)) { delete b; LH_FAIL(ctx, LH_EINVAL, "lh_batch_create: pod %u is not a stage of the same model as pod 0", i); }
            for (uint32_t j = 0; j < i; ++j)
                if (b->pods[j]->md.kc == p->md.kc || b->pods[j]->md.vc == p->md.vc) { delete b; LH_FAIL(ctx, LH_EINVAL, "lh_batch_create: pods %u and %u share a KV cache", j, i); }
        }
        b->pods.push_back(p);
    }
    Plan* p0 = b->pods[0];
    const ModelDesc& m = p0->md;
    b->batched = plan_batch_rows_ok(p0, n_pods);
    int rc = 0;
    if (b->batched) rc = plan_ensure_rows(p0, n_pods);
    else for (uint32_t i = 0; i < n_pods && !rc; ++i) rc = plan_ensure_rows(b->pods[i], 1);
    if (rc) { batch_free(b); return rc; }
    b->out_cap = m.ctx + 1;
    auto al = [&](void** ptr, size_t bytes) { return hipMalloc(ptr, bytes) == hipSuccess && hipMemsetAsync(*ptr, 0, bytes, ctx->stream) == hipSuccess; };
    bool ok = al((void**)&b->rows_dev, sizeof(BatchRow) * n_pods) && al((void**)&b->tok_dev, 4 * (size_t)n_pods) && al((void**)&b->ids_dev, 4 * (size_t)n_pods) &&
              al((void**)&b->sp_dev, sizeof(StepParams) * n_pods);
    if (ok && m.last_stage()) ok = al((void**)&b->out_dev, 4 * (size_t)n_pods * b->out_cap);
    if (ok && m.last_stage() && !b->batched && n_pods > 1) ok = al((void**)&b->logits_own, 4 * (size_t)n_pods * m.V);
    if (ok && b->batched && p0->attn_part) ok = al((void**)&b->attn_part, 4 * (size_t)n_pods * m.H * ((m.ctx + ATT_TC - 1) / ATT_TC) * (m.hd + 2));
    // prefix sharing: the block table of the shared tick kernel, where ticks have split partials to share (elsewhere a fork still copies and ticks run as ever)
    b->sh_gid.assign(n_pods, Batch::SH_NONE);
    b->sh_len.assign(n_pods, 0u);
    memset(&b->share_sent, 0, sizeof b->share_sent);
    for (uint32_t j = 0; j < SHARE_ROWS_MAX; ++j) b->share_sent.row_block[j] = SHARE_NO_BLOCK;
    if (ok && b->attn_part && m.first_stage() && m.last_stage())
        ok = al((void**)&b->share_dev, sizeof(ShareTable)) && hipMemsetAsync(b->share_dev, 0xFF, sizeof(ShareTable), ctx->stream) == hipSuccess;   // every row: no block
    if (ok) {
        // The zero fills above run on the context's stream, which is non-blocking: a synchronous copy (null stream) is NOT ordered behind
        // them.  Without this wait the fill of rows_dev could land after the table below and leave null cache pointers in it (seen as a GPU
        // memory fault at cache position 8 x embd, twice in ~40 two-rank runs of round 3).
        ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
        std::vector<BatchRow> hr(n_pods);
        for (uint32_t i = 0; i < n_pods; ++i) hr[i] = BatchRow{b->pods[i]->md.kc, b->pods[i]->md.vc, 0u, 0u};
        ok = ok && hipMemcpy(b->rows_dev, hr.data(), sizeof(BatchRow) * n_pods, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipGetLastError(); batch_free(b); LH_FAIL(ctx, LH_ENOMEM, "lh_batch_create: device allocation failed"); }
    lh_batch* h = new lh_batch();
    h->b = b;
    *out = h;
    return LH_OK;
}

void lh_batch_destroy(lh_batch* h) {
    if (!h) return;
    batch_free(h->b);
    delete h;
}

uint32_t lh_batch_rows(const lh_batch* h) { return h ? h->b->B : 0; }
int lh_batch_batched(const lh_batch* h) { return h && h->b->batched ? 1 : 0; }
uint32_t* lh_batch_tokens_dev(lh_batch* h) { return h ? h->b->tok_dev : nullptr; }
uint32_t* lh_batch_ids_dev(lh_batch* h) { return h ? h->b->ids_dev : nullptr; }

int lh_batch_read_ids(lh_batch* h, uint32_t* ids_host) {
    if (!h || !ids_host) return LH_EINVAL;
    lh_ctx* ctx = h->b->ctx;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    LH_HIP(ctx, hipMemcpyAsync(ids_host, h->b->ids_dev, (size_t)h->b->B * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

int lh_batch_set(lh_batch* h, const uint32_t* tokens, const uint32_t* past) {
    if (!h || !past) return LH_EINVAL;
    LH_HIP(h->b->ctx, hipSetDevice(h->b->ctx->device));
    int rc = batch_set(h->b, tokens, past);
    if (rc == 0) for (uint32_t i = 0; i < h->b->B; ++i) share_written(h->b, i, past[i]);   // placed below a shared length: the next tick writes there
    return rc;
}

int lh_batch_set_sampler(lh_batch* h, const lh_sample_params* sp, uint32_t ring_size, const uint32_t* const* ring_init, const uint32_t* n_init) {
    if (!h) return LH_EINVAL;
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!sp) { b->sampling = false; return LH_OK; }   // back to greedy ticks
    if (!m.last_stage()) { b->sampling = false; return LH_OK; }   // only the last stage samples; the other stages' ticks are the same either way
    int rc;
    if ((rc = sample_check(ctx, sp, m.V))) return rc;
    if (ring_size == 0) LH_FAIL(ctx, LH_EINVAL, "lh_batch_set_sampler: the lastNTokens ring needs at least one slot (the reference uses CtxSize, server.go:127)");
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!b->ss_dev) LH_HIP(ctx, hipMalloc((void**)&b->ss_dev, sizeof(SampleState) * b->B));
    if ((rc = grow(ctx, &b->ring_dev, &b->ring_cap, ring_size, (size_t)b->B * 4, 0, &b->smp_gen))) return rc;   // (an element = one slot of every pod's ring)
    if ((sp->top_k <= 64) != (b->smp_topk <= 64)) b->smp_gen++;   // the captured tick holds the kernel variant
    b->smp_topk = sp->top_k;
    b->ring_size = ring_size;
    // ring: ring_size zeros, then the ids seen so far (appendToken, server.go:129-138, 193-197)
    std::vector<uint32_t> ring((size_t)b->B * b->ring_cap, 0u);
    std::vector<SampleState> st(b->B);
    for (uint32_t i = 0; i < b->B; ++i) {
        const uint32_t ni = (ring_init && n_init) ? n_init[i] : 0;
        for (uint32_t j = 0; j < ni; ++j) ring[(size_t)i * b->ring_cap + j % ring_size] = ring_init[i][j];
        st[i] = SampleState{sp->top_k, sp->top_p, sp->temp, sp->repeat_penalty, sp->seed, 0, ring_size, ni};   // every row = a solo run with this seed
    }
    LH_HIP(ctx, hipMemcpy(b->ring_dev, ring.data(), ring.size() * 4, hipMemcpyHostToDevice));
    LH_HIP(ctx, hipMemcpy(b->ss_dev, st.data(), sizeof(SampleState) * b->B, hipMemcpyHostToDevice));
    // the rows' output lists restart (.step = index into them); token ids and positions stay what lh_batch_set / lh_batch_prompt / the ticks made
    // them.  The HOST mirror restarts with them: what the ticks so far produced is read first (the histories of the context swap and
    // each row's pending token), then the mirror is re-based on "tick 0 evaluates the pending token and writes entry 0" - the call may come
    // mid-stream, behind a prompt and any number of ticks.
    if (b->step0 + b->ticks > 0) {
        if ((rc = batch_drain(b))) return rc;
        b->pos_set = b->pos;
        b->tok0 = b->pending;
        b->tok0_known = true;
        b->step0 = 0; b->ticks = 0; b->drained = 0;
    }
    LH_LAUNCH(k_batch_reset_steps, dim3(1), dim3(64), 0, ctx->stream, b->rows_dev, b->sp_dev, b->B);
    LH_HIP(ctx, hipGetLastError());
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    b->sampling = true;
    return LH_OK;
}

int lh_batch_prompt(lh_batch* h, const uint32_t* const* prompts, const uint32_t* n_prompt, const float* x_in_dev, float* x_out_dev) {
    if (!h || !n_prompt) return LH_EINVAL;
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (m.first_stage() && !prompts) LH_FAIL(ctx, LH_EINVAL, "lh_batch_prompt: the first stage needs the prompts");
    if (!m.first_stage() && !x_in_dev) LH_FAIL(ctx, LH_EINVAL, "lh_batch_prompt: later stage needs the residual stream");
    if (!m.last_stage() && !x_out_dev) LH_FAIL(ctx, LH_EINVAL, "lh_batch_prompt: non-final stage needs an output buffer");
    uint32_t past[64];
    for (uint32_t i = 0; i < b->B; ++i) {   // everything is checked before anything runs
        if (!n_prompt[i] || n_prompt[i] > m.ctx) LH_FAIL(ctx, LH_EINVAL, "lh_batch_prompt: row %u: prompt of %u tokens outside 1..%u", i, n_prompt[i], m.ctx);
        if (m.first_stage()) {
            if (!prompts[i]) LH_FAIL(ctx, LH_EINVAL, "lh_batch_prompt: row %u has no prompt", i);
            for (uint32_t j = 0; j < n_prompt[i]; ++j)
                if (prompts[i][j] >= m.V) LH_FAIL(ctx, LH_EINVAL, "lh_batch_prompt: row %u: token id %u outside the vocabulary of %u", i, prompts[i][j], m.V);
        }
        past[i] = n_prompt[i];
    }
    int rc;
    for (uint32_t i = 0; i < b->B; ++i) share_written(b, i, 0);   // every pod's cache is rewritten from position 0: the sharing groups end
    LH_HIP(ctx, hipMemsetAsync(b->sp_dev, 0, sizeof(StepParams) * b->B, ctx->stream));   // sampling: the prompt's id is entry 0 of the row's output list
    size_t off = 0;   // rows of the pods, one after the other, in the residual stream buffers
    for (uint32_t i = 0; i < b->B; ++i) {
        Plan* p = b->pods[i];
        const uint32_t n = n_prompt[i];
        // the prompt as ONE Eval on the row's own plan (server.go:185-192).  (Plan 0 also holds the batch's scratch: it only ever grows, and
        // the captured tick is re-captured when it did - Plan::scratch_gen.)
        if ((rc = plan_eval(p, m.first_stage() ? prompts[i] : nullptr, x_in_dev ? x_in_dev + off * m.d : nullptr, x_out_dev ? x_out_dev + off * m.d : nullptr, n, 0, true))) return rc;
        if (m.last_stage()) {
            const float* last_row = n == 1 ? p->logits : p->logits + (size_t)(n - 1) * m.V;
            if (b->sampling) {
                if ((rc = sample_launch(ctx, last_row, m.V, b->ss_dev + i, b->ring_dev + (size_t)i * b->ring_cap, b->sp_dev + i, b->out_dev + (size_t)i * b->out_cap, b->ids_dev + i,
                                        nullptr, nullptr, nullptr, 1, b->smp_topk)))
                    return rc;
            } else {
                LH_LAUNCH(k_argmax_advance, dim3(1), dim3(1024), 0, ctx->stream, last_row, m.V, (StepParams*)nullptr, b->out_dev + (size_t)i * b->out_cap, b->ids_dev + i, 0);
                LH_HIP(ctx, hipMemcpyAsync(b->out_dev + (size_t)i * b->out_cap, b->ids_dev + i, 4, hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        off += n;
    }
    if (m.first_stage() && m.last_stage()) LH_HIP(ctx, hipMemcpyAsync(b->tok_dev, b->ids_dev, (size_t)b->B * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = batch_set(b, nullptr, past, 1))) return rc;   // every row now stands behind its prompt; out[row][0] holds the id the prompt produced
    LH_HIP(ctx, hipGetLastError());
    return LH_OK;
}

int lh_batch_stage(lh_batch* h, const float* x_in_dev, float* x_out_dev, float* logits_dev, uint32_t* ids_dev) {
    if (!h) return LH_EINVAL;
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!m.first_stage() && !x_in_dev) LH_FAIL(ctx, LH_EINVAL, "lh_batch_stage: later stage needs the residual stream");
    if (!m.last_stage() && !x_out_dev) LH_FAIL(ctx, LH_EINVAL, "lh_batch_stage: non-final stage needs an output buffer");
    int rc;
    if ((rc = batch_tick(b, x_in_dev, x_out_dev))) return rc;
    if (m.last_stage() && logits_dev) LH_HIP(ctx, hipMemcpyAsync(logits_dev, b->logits(), (size_t)b->B * m.V * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (m.last_stage() && ids_dev) LH_HIP(ctx, hipMemcpyAsync(ids_dev, b->ids_dev, (size_t)b->B * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return LH_OK;
}

int lh_batch_decode(lh_batch* h, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, uint32_t* out_tokens, float* logits_last_host) {
    if (!h || !first_tokens || !past || !n_steps) return LH_EINVAL;
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!m.first_stage() || !m.last_stage()) LH_FAIL(ctx, LH_EINVAL, "lh_batch_decode needs whole-model pods; use lh_batch_stage on a layer shard");
    int rc;
    if ((rc = batch_set(b, first_tokens, past))) return rc;
    b->collecting = true;
    b->gen.assign(b->B, std::vector<uint32_t>());
    for (uint32_t s = 0; s < n_steps && !rc; ++s) rc = batch_tick(b, nullptr, nullptr);   // (a row whose window is full swaps context first: batch_swap)
    if (!rc) rc = batch_drain(b);
    b->collecting = false;
    if (rc) return rc;
    if (out_tokens)
        for (uint32_t i = 0; i < b->B; ++i) memcpy(out_tokens + (size_t)i * n_steps, b->gen[i].data(), (size_t)n_steps * 4);
    if (logits_last_host) LH_HIP(ctx, hipMemcpyAsync(logits_last_host, b->logits(), (size_t)b->B * m.V * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

// lh_batch_decode_lookup and (smp) lh_batch_decode_sample_lookup: the checks, then the loop
static int batch_decode_lookup_checked(lh_batch* h, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out_tokens,
                                       float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap, bool smp) {
    if (!h) return LH_EINVAL;
    const char* who = smp ? "lh_batch_decode_sample_lookup" : "lh_batch_decode_lookup";
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // ---- everything is checked before anything is enqueued or any host state moves
    if (!first_tokens || !past || !out_tokens) LH_FAIL(ctx, LH_EINVAL, "%s: null argument", who);
    if (!n_steps) LH_FAIL(ctx, LH_EINVAL, "%s: no ids asked for", who);
    if (!m.first_stage() || !m.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "%s needs whole-model pods (layers [%u, %u) of %u)", who, m.layer0, m.layer1, m.L);
    if (!smp && b->sampling) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_batch_decode_lookup: the batch has a sampler set (greedy only; lh_batch_set_sampler(NULL) first)");
    if (smp && !b->sampling) LH_FAIL(ctx, LH_EINVAL, "lh_batch_decode_sample_lookup: the batch has no sampler set (lh_batch_decode_lookup runs a greedy batch)");
    int rc;
    {   // draft_max is 1..7 for both weight types here: beyond the bit-identical rows the passes are batched Evals like a feed's
        if (!lp) LH_FAIL(ctx, LH_EINVAL, "%s: no lookup parameters", who);
        if (lp->draft_max < 1 || lp->draft_max > SPEC_ROWS_MAX - 1) LH_FAIL(ctx, LH_EINVAL, "%s: draft_max %u (1..%u)", who, lp->draft_max, SPEC_ROWS_MAX - 1);
        lh_lookup_params one = *lp;
        one.draft_max = 1;
        if ((rc = spec_check_params(ctx, m, &one, who))) return rc;
    }
    const uint32_t R = batch_spec_rows(b, lp->draft_max);
    for (uint32_t i = 0; i < b->B; ++i) {
        if (first_tokens[i] >= m.V) LH_FAIL(ctx, LH_EINVAL, "%s: token id %u of row %u outside the vocabulary of %u", who, first_tokens[i], i, m.V);
        if ((uint64_t)past[i] + n_steps + R - 1 > m.ctx)
            LH_FAIL(ctx, LH_EINVAL, "%s: row %u: past %u + n_steps %u + %u rows per pass - 1 exceeds the context window of %u (the loop never leaves the window)", who,
                    i, past[i], n_steps, R, m.ctx);
    }
    if (R == 1) {   // no multi-row pass for this pod count on this plan's shapes: plain ticks, and the stats say so
        if ((rc = lh_batch_decode(h, first_tokens, past, n_steps, out_tokens, logits_last_host))) return rc;
        for (uint32_t i = 0; i < b->B; ++i) {
            if (stats) stats[i] = lh_spec_stats{n_steps, 1, 0, 0, n_steps};
            if (trace) for (uint32_t t = 0; t < n_steps && t < trace_cap; ++t) trace[(size_t)i * trace_cap + t] = 0;
        }
        return LH_OK;
    }
    for (uint32_t i = 0; i < b->B; ++i) share_written(b, i, past[i]);   // the passes write every pod's cache from past[i] on
    return batch_decode_lookup(b, first_tokens, past, n_steps, lp, R, out_tokens, logits_last_host, stats, trace, trace_cap, smp);
}

int lh_batch_decode_lookup(lh_batch* h, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out_tokens,
                           float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    return batch_decode_lookup_checked(h, first_tokens, past, n_steps, lp, out_tokens, logits_last_host, stats, trace, trace_cap, false);
}

int lh_batch_decode_sample_lookup(lh_batch* h, const uint32_t* first_tokens, const uint32_t* past, uint32_t n_steps, const lh_lookup_params* lp, uint32_t* out_tokens,
                                  float* logits_last_host, lh_spec_stats* stats, uint16_t* trace, uint32_t trace_cap) {
    return batch_decode_lookup_checked(h, first_tokens, past, n_steps, lp, out_tokens, logits_last_host, stats, trace, trace_cap, true);
}

uint32_t lh_batch_sampler_ring_size(const lh_batch* h) { return h && h->b->sampling ? h->b->ring_size : 0u; }

int lh_batch_sampler_read(lh_batch* h, uint32_t pod, uint32_t* ring_out, uint32_t* ring_pos_out, uint64_t* draw_out) {
    if (!h) return LH_EINVAL;
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!b->sampling) LH_FAIL(ctx, LH_EINVAL, "lh_batch_sampler_read: the batch has no sampler set");
    if (pod >= b->B) LH_FAIL(ctx, LH_EINVAL, "lh_batch_sampler_read: pod %u outside the batch of %u", pod, b->B);
    SampleState st;
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    LH_HIP(ctx, hipMemcpy(&st, b->ss_dev + pod, sizeof st, hipMemcpyDeviceToHost));
    if (ring_out) LH_HIP(ctx, hipMemcpy(ring_out, b->ring_dev + (size_t)pod * b->ring_cap, (size_t)st.ring_size * 4, hipMemcpyDeviceToHost));
    if (ring_pos_out) *ring_pos_out = st.ring_pos;
    if (draw_out) *draw_out = st.draw;
    return LH_OK;
}

// lh_spec_accept_pods and (rings != nullptr) lh_spec_accept_sample_pods: one k_spec_accept_pods launch on host arrays
static int spec_accept_pods_host(lh_ctx* ctx, const char* who, const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos,
                                 const uint32_t* produced, uint32_t n_steps, uint32_t ctx_size, const uint32_t* rings, uint32_t ring_size, const uint32_t* ring_pos,
                                 const uint64_t* draws, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out, uint32_t* pending_out, uint32_t* ids_out,
                                 uint32_t* rings_out, uint32_t* ring_pos_out, uint64_t* draws_out) {
    if (!ctx) return LH_EINVAL;
    if (!arg || !tok || !k || !pos || !produced || !a_out || !pos_out || !produced_out || !pending_out || !ids_out) LH_FAIL(ctx, LH_EINVAL, "%s: null argument", who);
    const uint32_t P = n_pods, R = n_rows;
    if (P < 1 || P > BATCH_ROWS_MAX || R < 1 || R > SPEC_ROWS_MAX || P * R > BATCH_ROWS_MAX)
        LH_FAIL(ctx, LH_EINVAL, "%s: %u pods x %u rows (1..%u pods, 1..%u rows, at most %u rows in all)", who, P, R, BATCH_ROWS_MAX, SPEC_ROWS_MAX, BATCH_ROWS_MAX);
    if (!ctx_size) LH_FAIL(ctx, LH_EINVAL, "%s: an empty window", who);
    if (rings && !ring_size) LH_FAIL(ctx, LH_EINVAL, "%s: the lastNTokens ring needs at least one slot", who);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: arg | tok | pending | output lists [P][R] | states | summaries | row table | sampler states | rings
    const size_t n = (size_t)P * R, o_tok = 4 * n, o_pend = o_tok + 4 * n, o_out = o_pend + 4 * (size_t)P, o_st = (o_out + 4 * n + 63) & ~(size_t)63,
                 o_sum = o_st + sizeof(SpecState) * P, o_rows = o_sum + sizeof(SpecPodSum) * P, o_ss = (o_rows + sizeof(BatchRow) * n + 63) & ~(size_t)63,
                 o_ring = o_ss + (rings ? sizeof(SampleState) * P : 0), total = o_ring + (rings ? 4 * (size_t)P * ring_size : 0);
    std::vector<char> hb(total, 0);
    if (rings) {
        memcpy(hb.data() + o_ring, rings, 4 * (size_t)P * ring_size);
        for (uint32_t i = 0; i < P; ++i) {   // only the ring and the two counters are read by the commit
            SampleState* ss = (SampleState*)(hb.data() + o_ss) + i;
            ss->ring_size = ring_size; ss->ring_pos = ring_pos[i]; ss->draw = draws[i];
        }
    }
    memcpy(hb.data(), arg, 4 * n);
    memcpy(hb.data() + o_tok, tok, 4 * n);
    std::vector<uint32_t> base(P);   // a pod's list holds only what this pass appends: entry `produced` of the loop's list is entry 0 here
    for (uint32_t i = 0; i < P; ++i) {
        ((uint32_t*)(hb.data() + o_pend))[i] = tok[(size_t)i * R];
        SpecState* st = (SpecState*)(hb.data() + o_st) + i;
        base[i] = std::min(produced[i], n_steps);
        st->pos = pos[i]; st->produced = produced[i] - base[i]; st->n_steps = n_steps - base[i]; st->k = k[i];
    }
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    hipError_t e = hipMemcpyAsync(dev, hb.data(), total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) {
        SpecPodsArgs a = {};
        a.arg = (const uint32_t*)dev; a.tok = (uint32_t*)(dev + o_tok); a.pend = (uint32_t*)(dev + o_pend); a.out = (uint32_t*)(dev + o_out); a.st = (SpecState*)(dev + o_st);
        a.sum = (SpecPodSum*)(dev + o_sum); a.rows = (BatchRow*)(dev + o_rows);
        a.R = R; a.ctx = ctx_size; a.vocab = SPEC_UNKNOWN; a.out_cap = R;
        if (rings) { a.ss = (SampleState*)(dev + o_ss); a.ring = (uint32_t*)(dev + o_ring); a.ring_cap = ring_size; }
        const SpecLookup none = {nullptr, 0, 0, 1, 1};
        LH_LAUNCH(k_spec_accept_pods, dim3(P), dim3(SPEC_TH), 0, ctx->stream, a, none, 0);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), dev, total, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "%s: %s", who, hipGetErrorString(e));
    if (rings && rings_out) memcpy(rings_out, hb.data() + o_ring, 4 * (size_t)P * ring_size);
    for (uint32_t i = 0; i < P; ++i) {
        if (rings) {
            const SampleState* ss = (const SampleState*)(hb.data() + o_ss) + i;
            if (ring_pos_out) ring_pos_out[i] = ss->ring_pos;
            if (draws_out) draws_out[i] = ss->draw;
        }
        const SpecState* st = (const SpecState*)(hb.data() + o_st) + i;
        a_out[i] = st->last_a; pos_out[i] = st->pos; produced_out[i] = st->produced + base[i];
        pending_out[i] = ((const uint32_t*)(hb.data() + o_pend))[i];
        const uint32_t appended = st->produced - (produced[i] - base[i]);
        for (uint32_t j = 0; j < R; ++j) ids_out[(size_t)i * R + j] = j < appended ? ((const uint32_t*)(hb.data() + o_out))[(size_t)i * R + j] : SPEC_UNKNOWN;
    }
    return LH_OK;
}

int lh_spec_accept_pods(lh_ctx* ctx, const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos,
                        const uint32_t* produced, uint32_t n_steps, uint32_t ctx_size, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out, uint32_t* pending_out,
                        uint32_t* ids_out) {
    return spec_accept_pods_host(ctx, "lh_spec_accept_pods", arg, tok, n_pods, n_rows, k, pos, produced, n_steps, ctx_size, nullptr, 0, nullptr, nullptr, a_out, pos_out,
                                 produced_out, pending_out, ids_out, nullptr, nullptr, nullptr);
}

int lh_spec_accept_sample_pods(lh_ctx* ctx, const uint32_t* arg, const uint32_t* tok, uint32_t n_pods, uint32_t n_rows, const uint32_t* k, const uint32_t* pos,
                               const uint32_t* produced, uint32_t n_steps, uint32_t ctx_size, const uint32_t* rings, uint32_t ring_size, const uint32_t* ring_pos,
                               const uint64_t* draws, uint32_t* a_out, uint32_t* pos_out, uint32_t* produced_out, uint32_t* pending_out, uint32_t* ids_out,
                               uint32_t* rings_out, uint32_t* ring_pos_out, uint64_t* draws_out) {
    if (!ctx) return LH_EINVAL;
    if (!rings || !ring_pos || !draws) LH_FAIL(ctx, LH_EINVAL, "lh_spec_accept_sample_pods: null argument");
    return spec_accept_pods_host(ctx, "lh_spec_accept_sample_pods", arg, tok, n_pods, n_rows, k, pos, produced, n_steps, ctx_size, rings, ring_size, ring_pos, draws, a_out,
                                 pos_out, produced_out, pending_out, ids_out, rings_out, ring_pos_out, draws_out);
}

int lh_batch_feed(lh_batch* h, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past, uint32_t* ids_host, float* logits_last_host,
                  float* logits_rows_host) {
    if (!h || !n_tokens) return LH_EINVAL;
    LH_HIP(h->b->ctx, hipSetDevice(h->b->ctx->device));
    return batch_feed(h->b, tokens, n_tokens, past, nullptr, false, ids_host, logits_last_host, logits_rows_host);
}

int lh_batch_feed_sample(lh_batch* h, const uint32_t* const* tokens, const uint32_t* n_tokens, const uint32_t* past, const uint32_t* flags, uint32_t* ids_host,
                         float* logits_last_host, float* logits_rows_host) {
    if (!h || !n_tokens) return LH_EINVAL;
    LH_HIP(h->b->ctx, hipSetDevice(h->b->ctx->device));
    return batch_feed(h->b, tokens, n_tokens, past, flags, true, ids_host, logits_last_host, logits_rows_host);
}

int lh_feed_schedule(const uint32_t* n_tokens, const uint32_t* past, uint32_t rows, uint32_t solo_min, uint32_t qb, uint64_t sizes_ok, lh_feed_pass* passes,
                     uint32_t pass_cap, lh_feed_seg* segs, uint32_t seg_cap, lh_feed_block* blocks, uint32_t block_cap, uint32_t* counts) {
    if (!n_tokens || !past || !rows || rows > 64 || !qb || !solo_min) return -1;
    FeedSchedule fs;
    feed_schedule(n_tokens, past, rows, solo_min, qb, sizes_ok, &fs);
    for (size_t i = 0; passes && i < fs.passes.size() && i < pass_cap; ++i) passes[i] = fs.passes[i];
    for (size_t i = 0; segs && i < fs.segs.size() && i < seg_cap; ++i) segs[i] = fs.segs[i];
    for (size_t i = 0; blocks && i < fs.blocks.size() && i < block_cap; ++i) blocks[i] = fs.blocks[i];
    if (counts) { counts[0] = (uint32_t)fs.passes.size(); counts[1] = (uint32_t)fs.segs.size(); counts[2] = (uint32_t)fs.blocks.size(); }
    return (int)fs.passes.size();
}

// ---- lh_batch_fork: a pod's evaluated prefix for other pods of the batch (llamahip.h states the rule) -------------------------------------------------
int lh_batch_fork(lh_batch* h, uint32_t src, const uint32_t* dst, uint32_t n_dst, uint32_t n_pos) {
    if (!h) return LH_EINVAL;
    Batch* b = h->b;
    lh_ctx* ctx = b->ctx;
    const ModelDesc& m = b->pods[0]->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // ---- everything is checked before anything is enqueued or any host state moves
    if (!m.first_stage() || !m.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_batch_fork needs whole-model pods (layers [%u, %u) of %u)", m.layer0, m.layer1, m.L);
    if (!dst || !n_dst) LH_FAIL(ctx, LH_EINVAL, "lh_batch_fork: no destination pod");
    if (!n_pos) LH_FAIL(ctx, LH_EINVAL, "lh_batch_fork: no position to copy");
    if (src >= b->B) LH_FAIL(ctx, LH_EINVAL, "lh_batch_fork: source pod %u outside the batch of %u", src, b->B);
    uint64_t seen = 1ull << src;
    for (uint32_t i = 0; i < n_dst; ++i) {
        if (dst[i] >= b->B) LH_FAIL(ctx, LH_EINVAL, "lh_batch_fork: destination pod %u outside the batch of %u", dst[i], b->B);
        if (seen & (1ull << dst[i])) LH_FAIL(ctx, LH_EINVAL, "lh_batch_fork: pod %u is the source or named twice", dst[i]);
        seen |= 1ull << dst[i];
    }
    if (!b->pos_known || n_pos > b->pos[src])
        LH_FAIL(ctx, LH_EINVAL, "lh_batch_fork: %u positions, the source pod %u stands at %u (the host mirror; not placed yet: 0)", n_pos, src, b->pos_known ? b->pos[src] : 0u);
    int rc;
    // Tokens the ticks evaluated are recorded in the histories only when the host next reads the ids (batch_drain).  Read them NOW, whatever the
    // positions: the source's copied range may need them, and a destination's undrained ticks would otherwise be recorded LATER, at its old positions,
    // over the history copied below - a later context swap would then re-feed tokens its cache no longer holds.
    if (b->ticks > b->drained && (rc = batch_drain(b))) return rc;
    share_sync(b);
    // ---- the copy, in stream order: rows [0, n_pos) of every layer slot of [layers][ctx][d], K and V
    const Plan* sp = b->pods[src];
    const size_t pitch = (size_t)m.ctx * m.d * 4, width = (size_t)n_pos * m.d * 4, layers = m.layer1 - m.layer0;
    for (uint32_t i = 0; i < n_dst; ++i) {
        Plan* dp = b->pods[dst[i]];
        LH_HIP(ctx, hipMemcpy2DAsync(dp->md.kc, pitch, sp->md.kc, pitch, width, layers, hipMemcpyDeviceToDevice, ctx->stream));
        LH_HIP(ctx, hipMemcpy2DAsync(dp->md.vc, pitch, sp->md.vc, pitch, width, layers, hipMemcpyDeviceToDevice, ctx->stream));
        if (sp->hist && dp->hist)
            for (uint32_t k = 0; k < n_pos && k < sp->hist->size() && k < dp->hist->size(); ++k) (*dp->hist)[k] = (*sp->hist)[k];
    }
    // ---- the group {src} + dst of shared length n_pos: the destinations join src's group if it has exactly that length, else a new group forms
    if (b->sh_gid[src] != Batch::SH_NONE && b->sh_len[src] == n_pos) {
        const uint32_t gid = b->sh_gid[src];
        for (uint32_t i = 0; i < n_dst; ++i) {
            if (b->sh_gid[dst[i]] == gid) continue;
            // (leaving cannot dissolve src's group: a group that is not src's loses the pod)
            share_leave(b, dst[i]);
            share_set(b, dst[i], gid, n_pos);
        }
    } else {
        share_leave(b, src);
        for (uint32_t i = 0; i < n_dst; ++i) share_leave(b, dst[i]);
        const uint32_t gid = b->sh_next_gid++;
        share_set(b, src, gid, n_pos);
        for (uint32_t i = 0; i < n_dst; ++i) share_set(b, dst[i], gid, n_pos);
    }
    return LH_OK;
}

int lh_batch_share_info(lh_batch* h, uint32_t* group_out, uint32_t* len_out) {
    if (!h || !group_out || !len_out) return LH_EINVAL;
    share_info(h->b, group_out, len_out);
    return LH_OK;
}

int lh_batch_share_written(lh_batch* h, uint32_t pod, uint32_t pos_lo) {
    if (!h || pod >= h->b->B) return LH_EINVAL;
    share_written(h->b, pod, pos_lo);
    return LH_OK;
}

int lh_share_schedule(const uint32_t* group, const uint32_t* len, uint32_t rows, uint32_t qb, uint32_t min_rows, lh_share_block* blocks, uint32_t cap, uint32_t* row_block) {
    return share_schedule(group, len, rows, qb, min_rows, blocks, cap, row_block);
}

int lh_llama_profile_decode(lh_llama* m, uint32_t token, uint32_t past, uint32_t repeats, lh_kernel_time* out, uint32_t cap) {
    if (!m || !out || !repeats) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure_out_tokens(p, 1))) return rc;
    const float* pin = p->md.first_stage() ? nullptr : p->h;   // stage models: scratch stands in for the received residual
    float* pout = p->md.last_stage() ? nullptr : p->attn;
    ProfSink sink;
    sink.on = true;
    // warm-up (also sets kernel attributes), then timed eager steps at the same position
    g_prof = nullptr;
    if ((rc = upload_step_params(p, 0, token, past, 0))) return rc;
    if ((rc = enqueue_decode(p, p->sp_dev, pin, pout, false, nullptr))) return rc;
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    g_prof = &sink;
    LH_LAUNCH(k_park, dim3(1), dim3(1), 0, ctx->stream, (uint64_t)(repeats * 1500000ull));  // 15 ms per repeat of host queueing time
    for (uint32_t r = 0; r < repeats && !rc; ++r) rc = enqueue_decode(p, p->sp_dev, pin, pout, false, p->md.last_stage() ? p->argmax_dev : nullptr);
    g_prof = nullptr;
    hipStreamSynchronize(ctx->stream);
    std::vector<lh_kernel_time> acc;
    for (auto& r : sink.recs) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        hipEventDestroy(r.e0);
        hipEventDestroy(r.e1);
        size_t i = 0;
        for (; i < acc.size(); ++i) if (!strcmp(acc[i].name, r.name)) break;
        if (i == acc.size()) {
            lh_kernel_time t = {};
            snprintf(t.name, sizeof t.name, "%s", r.name);
            t.bytes_per_launch = r.bytes;
            acc.push_back(t);
        }
        acc[i].launches += 1;
        acc[i].total_ms += ms;
    }
    if (rc) return rc;
    // Second pass for the dominant weight-stream kernel: all of its launches of a step (one per layer, all weights distinct)
    // back to back between ONE event pair, queued behind the park kernel.  The per-kernel pairs above carry ~3 us of event
    // processing each; this is the figure that agrees with a rocprofv3 kernel trace (entry "<name>/b2b").
    size_t dom = acc.size();
    for (size_t i = 0; i < acc.size(); ++i)
        if (!strncmp(acc[i].name, "gemv_", 5) && (dom == acc.size() || acc[i].total_ms > acc[dom].total_ms)) dom = i;
    if (dom < acc.size() && acc[dom].launches >= repeats) {
        static thread_local char only_name[48];
        snprintf(only_name, sizeof only_name, "%s", acc[dom].name);
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        g_only = only_name;
        LH_LAUNCH(k_park, dim3(1), dim3(1), 0, ctx->stream, (uint64_t)(repeats * 300000ull));
        hipEventRecord(e0, ctx->stream);
        for (uint32_t r = 0; r < repeats && !rc; ++r) rc = enqueue_decode(p, p->sp_dev, pin, pout, false, nullptr);
        hipEventRecord(e1, ctx->stream);
        g_only = nullptr;
        hipStreamSynchronize(ctx->stream);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        hipEventDestroy(e0);
        hipEventDestroy(e1);
        if (rc) return rc;
        lh_kernel_time t = {};
        snprintf(t.name, sizeof t.name, "%s/b2b", acc[dom].name);
        t.bytes_per_launch = acc[dom].bytes_per_launch;
        t.launches = acc[dom].launches;
        t.total_ms = ms;
        acc.push_back(t);
    }
    uint32_t n = (uint32_t)std::min<size_t>(acc.size(), cap);
    for (uint32_t i = 0; i < n; ++i) out[i] = acc[i];
    return (int)n;
}

}  // extern "C"
