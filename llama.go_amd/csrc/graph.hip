// csrc/graph.hip — lh_graph_compute: the replacement of ml.GraphCompute (pkg/ml/ml.go:1411-1528).
//
// 1. resolve storage (persistent buffers, per-graph scratch arena, view offsets);
// 2. recognise the graph llama.Eval builds (pkg/llama/llama.go:211-389) by STRUCTURE (walking src0/src1 from
//    the final node) and run it as a fused plan (plan.hip);
// 3. otherwise — or with LH_GRAPH_NO_FUSION — run node by node, one kernel per op, exactly like the reference's
//    sequential walk (INIT/FINALIZE phases are no-ops for every implemented op, ml.go:1501-1526).
#include "plan.h"
#include <chrono>
#include "kernels_generic.h"
#include "graph_check.h"
#include "graph_match.h"
#include <math.h>
#include <algorithm>

namespace lh {

int gemm_small_n(lh_ctx* ctx, const float* w, const float* x, float* y, const float* resid, uint32_t M, uint32_t K, uint32_t n,
                 uint32_t ldx, uint32_t ldy, const char* name, bool split_ok = true);  // plan.hip

enum { OP_NONE = 0, OP_ADD = 2, OP_MUL = 4, OP_REPEAT = 10, OP_SILU = 17, OP_RMS_NORM = 19, OP_MUL_MAT = 20, OP_SCALE = 21, OP_CPY = 22,
       OP_RESHAPE = 23, OP_VIEW = 24, OP_PERMUTE = 25, OP_TRANSPOSE = 26, OP_GET_ROWS = 27, OP_DIAG_MASK_INF = 28, OP_SOFT_MAX = 29, OP_ROPE = 30 };

static inline uint64_t nelem(const lh_tensor& t) { return (uint64_t)t.ne[0] * t.ne[1] * t.ne[2] * t.ne[3]; }
static inline bool contiguous(const lh_tensor& t) {  // ml.go:206-211
    return t.nb[0] == 4 && t.nb[1] == t.nb[0] * t.ne[0] && t.nb[2] == t.nb[1] * t.ne[1] && t.nb[3] == t.nb[2] * t.ne[2];
}

// ---------------------------------------------------------------------------------------------------
// Structural matcher for the graph of llama.Eval: csrc/graph_match.h (pure host code, also behind lh_graph_match).  Here its buffer lookup is
// the context's snapshot of the device's table, and what it extracted is resolved to device pointers.
// ---------------------------------------------------------------------------------------------------
struct CtxLookup {
    lh_ctx* ctx;
    bool operator()(lh_buf id, gm::BufInfo* out) const {
        const Buffer* b = find_buffer_fast(ctx, id);
        if (!b) return false;
        out->nfloats = b->nfloats; out->dtype = b->dtype; out->rows = b->rows; out->cols = b->cols; out->has_shape = true;
        return true;
    }
};
static bool model_desc_of(lh_ctx* ctx, const lh_tensor* T, const gm::MatchInfo& mi, ModelDesc* out) {
    ModelDesc& md = *out;
    md.V = mi.V; md.d = mi.d; md.H = mi.H; md.hd = mi.hd; md.L = mi.L; md.F = mi.F; md.ctx = mi.ctx;
    md.layer0 = 0; md.layer1 = md.L; md.cache_layer0 = 0;
    md.wtype = mi.wtype;
    bool ok = true;
    auto dev = [&](int32_t leaf, const float** scales) -> const float* {
        Buffer* b = find_buffer_fast(ctx, T[leaf].buf);
        if (!b) { ok = false; return nullptr; }
        if (scales) *scales = b->scales;
        return b->dev;
    };
    md.layers.assign(md.L, LayerW());
    for (uint32_t il = 0; il < md.L; ++il) {
        const int32_t* W = &mi.weights[(size_t)il * gm::W_PER_LAYER];
        LayerW& L = md.layers[il];
        L.attn_norm = dev(W[gm::W_ATTN_NORM], nullptr); L.ffn_norm = dev(W[gm::W_FFN_NORM], nullptr);
        L.wq = dev(W[gm::W_WQ], &L.s_wq); L.wk = dev(W[gm::W_WK], &L.s_wk); L.wv = dev(W[gm::W_WV], &L.s_wv); L.wo = dev(W[gm::W_WO], &L.s_wo);
        L.w1 = dev(W[gm::W_W1], &L.s_w1); L.w2 = dev(W[gm::W_W2], &L.s_w2); L.w3 = dev(W[gm::W_W3], &L.s_w3);
    }
    const int32_t* tail = &mi.weights[(size_t)md.L * gm::W_PER_LAYER];
    md.tok_emb = dev(tail[gm::W_TOK_EMB], nullptr); md.norm = dev(tail[gm::W_NORM], nullptr); md.output = dev(tail[gm::W_OUTPUT], &md.s_output);
    Buffer* kb = find_buffer_fast(ctx, T[mi.kc_owner].buf);
    Buffer* vb = find_buffer_fast(ctx, T[mi.vc_owner].buf);
    if (!ok || !kb || !vb || kb == vb) return false;
    md.kc = kb->dev;
    md.vc = vb->dev;
    if (!kb->kv_hist) kb->kv_hist = std::make_shared<std::vector<uint32_t>>();
    md.kv_hist = kb->kv_hist;   // the cache's token history (context swap of the generation loops): shared by every plan over this buffer
    return true;
}


// ---------------------------------------------------------------------------------------------------
// generic node-by-node execution
// ---------------------------------------------------------------------------------------------------
static TView view_of(const lh_tensor& t, float* p) {
    TView v;
    v.p = p;
    for (int i = 0; i < 4; ++i) { v.ne[i] = t.ne[i]; v.ns[i] = t.nb[i] / 4; }
    return v;
}
static inline dim3 grid_for(uint64_t total) { return dim3((unsigned)std::min<uint64_t>((total + 255) / 256, 65535)); }

static int run_node(lh_ctx* ctx, const lh_tensor* T, const std::vector<float*>& P, uint32_t i) {
    const lh_tensor& t = T[i];
    hipStream_t st = ctx->stream;
    auto V = [&](int k) { return view_of(T[k], P[k]); };
    switch (t.op) {
        case OP_NONE: case OP_RESHAPE: case OP_VIEW: case OP_PERMUTE: return 0;  // NOPs ml.go:1658-1663
        case OP_GET_ROWS: {
            const lh_tensor &a = T[t.src0], &b = T[t.src1];
            if (t.ne[0] != a.ne[0] || t.ne[1] != nelem(b) || a.nb[0] != 4) LH_FAIL(ctx, LH_ESHAPE, "[HALT]ComputeForwardGetRows : wrong dimensions!");
            if (b.host) {  // Go panics on src0.Data[r*NE[0]:] past the table (ml.go:1748); never let the GPU read out of range
                for (uint64_t k = 0; k < nelem(b); ++k)
                    if (!(b.host[k] >= 0.f) || (uint64_t)b.host[k] >= a.ne[1]) LH_FAIL(ctx, LH_EINVAL, "GetRows: row index %g outside the table of %u rows", (double)b.host[k], a.ne[1]);
            } else {
                LH_FAIL(ctx, LH_EUNSUPPORTED, "GetRows: indices must be a host leaf (they cannot be bounds-checked on the device)");
            }
            LH_LAUNCH(g_get_rows, dim3((unsigned)nelem(b)), dim3(256), 0, st, V(t.src0), V(t.src1), V(i));
            break;
        }
        case OP_RMS_NORM: {
            const lh_tensor& a = T[t.src0];
            LH_LAUNCH(g_rms_norm, dim3(a.ne[1] * a.ne[2] * a.ne[3]), dim3(256), 0, st, V(t.src0), V(i));
            break;
        }
        case OP_REPEAT: LH_LAUNCH(g_repeat, grid_for((uint64_t)t.ne[0] * t.ne[1]), dim3(256), 0, st, V(t.src0), V(i)); break;
        case OP_MUL: {
            const lh_tensor &a = T[t.src0], &b = T[t.src1];
            for (int k = 0; k < 4; ++k)
                if (a.ne[k] != b.ne[k] || a.ne[k] != t.ne[k]) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardMulFP32 : different shapes!");
            LH_LAUNCH(g_mul, grid_for(nelem(a)), dim3(256), 0, st, V(t.src0), V(t.src1), V(i));
            break;
        }
        case OP_ADD: {
            if (T[t.src1].nb[0] != 4) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardAddFP32 : [src1] is NOT contiguous!");
            LH_LAUNCH(g_add, grid_for(nelem(T[t.src0])), dim3(256), 0, st, V(t.src0), V(t.src1), V(i));
            break;
        }
        case OP_SILU: {
            if (!contiguous(T[t.src0])) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardSiluFP32 : [src0] is NOT contiguous!");
            if (!contiguous(t)) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardSiluFP32 : [dst] is NOT contiguous!");
            LH_LAUNCH(g_silu, grid_for(nelem(t)), dim3(256), 0, st, V(t.src0), V(i));
            break;
        }
        case OP_SCALE: {
            if (!contiguous(T[t.src0])) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardScaleFP32 : [src0] is NOT contiguous!");
            if (!contiguous(t)) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardScaleFP32 : [dst] is NOT contiguous!");
            LH_LAUNCH(g_scale, grid_for(nelem(t)), dim3(256), 0, st, V(i), (const float*)P[t.src1]);
            break;
        }
        case OP_CPY: {
            const lh_tensor& a = T[t.src0];
            if (!contiguous(t)) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardDupFP32 : [dst] is NOT contiguous!");
            if (nelem(t) != nelem(a)) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardDupFP32 : [dst] and [src0] capacities are different!");
            LH_LAUNCH(g_cpy, grid_for(nelem(a)), dim3(256), 0, st, V(t.src0), P[i], nelem(a));
            break;
        }
        case OP_DIAG_MASK_INF: LH_LAUNCH(g_diag_mask_inf, grid_for(nelem(t)), dim3(256), 0, st, V(i), (const float*)P[t.src1]); break;
        case OP_SOFT_MAX: {
            if (!contiguous(T[t.src0])) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardSoftMaxFP32 : [src0] is NOT contiguous!");
            if (!contiguous(t)) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardSoftMaxFP32 : [dst] is NOT contiguous!");
            LH_LAUNCH(g_soft_max, dim3(t.ne[1] * t.ne[2] * t.ne[3]), dim3(256), 0, st, V(i));
            break;
        }
        case OP_ROPE: {
            // src0's NE and NB address both sides (ml.go:2274-2281); dst is a ViewTensor of src0 (ml.go:1016): the same data, under packed strides
            // of its own when src0 is a permuted view, and those are never read
            const lh_tensor &a = T[t.src0], &b = T[t.src1];
            if (nelem(b) != 3 || !b.host) LH_FAIL(ctx, LH_ESHAPE, "[HALT] ComputeForwardRopeFP32 : src1 has NOT EXACT 3 elements!");
            const uint32_t past = (uint32_t)b.host[0], dims = (uint32_t)b.host[1], mode = (uint32_t)b.host[2];
            if (dims == 0 || dims % 2 || dims > a.ne[0]) LH_FAIL(ctx, LH_ESHAPE, "Rope: dims %u not supported", dims);
            const uint32_t maxpos = (mode == 0 ? past : 0) + a.ne[2];
            const double2* table = nullptr;
            int rc = ensure_rope_table(ctx, maxpos + 1, dims, &table);
            if (rc) return rc;
            const uint64_t total = (uint64_t)a.ne[3] * a.ne[2] * a.ne[1] * (dims / 2);
            LH_LAUNCH(g_rope, grid_for(total), dim3(256), 0, st, view_of(a, P[i]), table, past, dims, mode);
            break;
        }
        case OP_MUL_MAT: {
            const lh_tensor &a = T[t.src0], &b = T[t.src1];
            if (a.ne[0] != b.ne[0] || a.ne[2] != b.ne[2] || a.ne[3] != b.ne[3]) LH_FAIL(ctx, LH_ESHAPE, "MulMat: incompatible shapes (ml.go:290-292)");
            if (a.nb[0] != 4 || b.nb[0] != 4) LH_FAIL(ctx, LH_ESHAPE, "MulMat: operands must be contiguous along K (ml.go:1950, 1967)");
            if (a.dtype != 0) LH_FAIL(ctx, LH_EUNSUPPORTED, "MulMat: %s weights are only supported inside the fused LLaMA plan", a.dtype == 1 ? "f16" : a.dtype == 2 ? "block-int4" : "block-int8");
            const bool plain2d = contiguous(a) && contiguous(b) && contiguous(t) && a.ne[2] == 1 && a.ne[3] == 1 && b.ne[2] == 1 && b.ne[3] == 1 &&
                                 a.ne[0] % 4 == 0 && a.ne[0] <= 24576 && a.ne[1] >= 256;
            if (plain2d) {
                // the long-prompt GEMM on the bf16 pipe (k_gemm_b9, N > 128 rows) multiplies exactly only values in split_exact_values' range
                // (common.h): it takes operands the host has seen - host leafs scanned here, buffers whose uploads were scanned - and any
                // other MulMat runs on the fp32 GEMM, which gives the reference's IEEE results for inf, NaN and tiny values.  Decided
                // before anything is enqueued.
                auto seen_exact = [&](int32_t j) {
                    const lh_tensor& o = T[T[j].storage];
                    if (o.buf) { const Buffer* bb = find_buffer_fast(ctx, o.buf); return bb && !bb->unchecked.load(std::memory_order_relaxed); }
                    return o.op == OP_NONE && o.host && split_exact_values(o.host, nelem(o));
                };
                const bool split_ok = b.ne[1] > 128 && seen_exact(t.src0) && seen_exact(t.src1);
                return gemm_small_n(ctx, P[t.src0], P[t.src1], P[i], nullptr, a.ne[1], a.ne[0], b.ne[1], a.ne[0], a.ne[1], "mul_mat", split_ok);
            }
            const uint64_t outs = (uint64_t)a.ne[1] * a.ne[2] * a.ne[3] * b.ne[1];
            LH_TRACE("g_mul_mat");
            LH_LAUNCH(g_mul_mat, dim3((unsigned)((outs + 3) / 4)), dim3(256), 0, st, V(t.src0), V(t.src1), V(i));
            break;
        }
        default: LH_FAIL(ctx, LH_EUNSUPPORTED, "[HALT] Please implement : op %d (the reference halts on it too, ml.go:1536-1700)", (int)t.op);
    }
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace lh

using namespace lh;

extern "C" {

int lh_graph_compute(lh_ctx* ctx, const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, uint32_t flags) {
    if (!ctx || !T) return LH_EINVAL;
    static const bool timing = getenv("LLAMAHIP_TIMING") != nullptr;   // stderr: host phases of a fused Eval in microseconds
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return (long)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1000.0; };
    const auto tq0 = now();
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!n_leafs && !n_nodes) return LH_OK;
    const uint32_t total = n_leafs + n_nodes;   // counts whose sum wraps are refused by the structural check below, before total is used
    // lh_ctx_time_computes: one event in front of everything this call puts on the stream, one behind it (mark_end, in front of the call's
    // last wait); the sums are taken when the call returns with both recorded
    struct ComputeTimer {
        lh_ctx* c; std::chrono::steady_clock::time_point t0;
        ~ComputeTimer() {
            if (!c->tc_on || !c->tc_end) return;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->tc_ev0, c->tc_ev1) != hipSuccess) return;
            c->tc_calls++; c->tc_dev_us += (double)ms * 1e3;
            c->tc_wall_us += (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() / 1e3;
        }
    } compute_timer{ctx, tq0};
    ctx->tc_end = false;
    if (ctx->tc_on) LH_HIP(ctx, hipEventRecord(ctx->tc_ev0, ctx->stream));
    auto mark_end = [&]() { if (ctx->tc_on && hipEventRecord(ctx->tc_ev1, ctx->stream) == hipSuccess) ctx->tc_end = true; };
    // ---- structural checks (graph_check.h): every index run_node, the matcher and the storage pass below use is in range after this
    ctx->last_ptr.clear();   // a refused graph leaves nothing for lh_node_read
    ctx->last_len.clear();
    {
        char why[256];
        const int bad = gc::graph_check_structure(T, n_leafs, n_nodes, why, sizeof why);
        if (bad) LH_FAIL(ctx, bad, "%s", why);
    }
    ctx->last_ptr.assign(total, nullptr);
    ctx->last_len.assign(total, 0);
    ctx->last_fused = 0;
    ctx->pre_index = -1;

    // ---- fused LLaMA plan?
    if (!(flags & LH_GRAPH_NO_FUSION)) {
        gm::Matcher<CtxLookup> mt(T, n_leafs, n_nodes, CtxLookup{ctx});
        const gm::MatchInfo& m = mt.mi;
        ModelDesc md;
        const auto tq1 = now();
        if (mt.run() && model_desc_of(ctx, T, m, &md)) {
            int rc = 0;
            const auto tq2 = now();
            Plan* p = plan_find_or_create(ctx, md, &rc);
            const auto tq3 = now();
            if (p) rc = plan_eval(p, m.tokens.data(), nullptr, nullptr, m.N, m.past, (flags & LH_GRAPH_LAST_ROW_LOGITS) != 0);
            const auto tq4 = now();
            if (!rc && m.emb_node >= 0 && (T[m.emb_node].flags & LH_T_OUTPUT)) {
                float* emb = nullptr;
                rc = plan_embeddings(p, m.N, &emb);   // the final norm * weight rows [N][embd] (the fused lm_head launches never write them out)
                if (!rc) { ctx->last_ptr[m.emb_node] = emb; ctx->last_len[m.emb_node] = (uint64_t)m.N * m.d; }
            }
            if (!rc && (flags & LH_GRAPH_LAST_ROW_LOGITS)) {
                // this caller reads row N - 1 of the final node and nothing else (llama.go:394-401): the row follows the kernels into pinned host
                // memory in front of the Eval's one synchronisation, and lh_node_read of that range is then a host copy (round 5: a second
                // synchronise + copy + synchronise cost ~20 us of the 4.5 ms a token takes through this route)
                const uint64_t V = m.V;
                if (ctx->out_pinned_floats < V) {
                    if (ctx->out_pinned) hipHostFree(ctx->out_pinned);
                    ctx->out_pinned = nullptr; ctx->out_pinned_floats = 0;
                    if (hipHostMalloc((void**)&ctx->out_pinned, V * 4, hipHostMallocDefault) == hipSuccess) ctx->out_pinned_floats = V;
                }
                if (ctx->out_pinned && hipMemcpyAsync(ctx->out_pinned, p->logits + (uint64_t)(m.N - 1) * V, V * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess) {
                    ctx->pre_index = (int64_t)total - 1; ctx->pre_off = (uint64_t)(m.N - 1) * V; ctx->pre_n = V;
                }
            }
            if (!rc) {
                mark_end();
                LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
                if (timing) fprintf(stderr, "[llamahip] graph_compute N=%u: validate %.1f us, match %.1f, find plan %.1f, enqueue %.1f, wait %.1f\n", m.N, us(tq0, tq1), us(tq1, tq2), us(tq2, tq3), us(tq3, tq4), us(tq4, now()));
                ctx->last_ptr[total - 1] = p->logits;  // [N][V], the final node's layout (ne0 = V, ne1 = N)
                ctx->last_len[total - 1] = (uint64_t)m.N * m.V;
                ctx->last_fused = 1;
                return LH_OK;
            }
            // Shapes outside what the fused kernels are built for (more rows per workgroup than threads, K beyond the register tile,
            // head widths the attention kernel cannot tile) are not an error of the caller: the reference's generic MulMat has no such
            // limits (ml.go:1976-2098), so the graph runs node by node instead.  It recomputes everything, cache writes included.
            if (rc != LH_EUNSUPPORTED && rc != LH_ESHAPE) return rc;
            LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }

    // ---- generic path: what every op will touch lies inside its owner (graph_check.h), then storage for every owner
    std::vector<uint64_t> need;  // floats per owner: a registered buffer's size, the nelem a host leaf uploads, a scratch owner's own span
    {
        std::vector<lh_buf_extent> ext;
        for (uint32_t i = 0; i < total; ++i) {
            if ((uint32_t)T[i].storage != i || !T[i].buf) continue;
            const Buffer* b = find_buffer(ctx->ds, T[i].buf);
            if (b) ext.push_back(lh_buf_extent{T[i].buf, b->nfloats, b->dtype});
        }
        char why[256];
        const int bad = gc::graph_check_reach(T, n_leafs, n_nodes, ext.data(), (uint32_t)ext.size(), why, sizeof why, &need);
        if (bad) {
            ctx->last_ptr.clear();
            ctx->last_len.clear();
            LH_FAIL(ctx, bad, "%s", why);
        }
    }
    std::vector<uint64_t> offs(total, 0);
    uint64_t arena = 0, stage = 0;
    std::vector<char> written(total, 0);   // owners a node of this graph writes into
    for (uint32_t i = 0; i < total; ++i)
        if (T[i].op != OP_NONE) written[T[i].storage] = 1;
    for (uint32_t i = 0; i < total; ++i) {
        if ((uint32_t)T[i].storage != i) continue;
        if (T[i].buf) {
            Buffer* b = find_buffer(ctx->ds, T[i].buf);
            if (!b) LH_FAIL(ctx, LH_EINVAL, "tensor %u: unknown buffer %llu", i, (unsigned long long)T[i].buf);
            if (written[i]) b->unchecked.store(true, std::memory_order_relaxed);
            continue;
        }
        offs[i] = arena;
        arena += (need[i] * 4 + 255) & ~(uint64_t)255;
        if (T[i].host) stage += (nelem(T[i]) * 4 + 15) & ~(uint64_t)15;
    }
    int rc;
    if ((rc = ensure_arena(ctx, arena + 256))) return rc;
    if ((rc = ensure_staging(ctx, stage + 16))) return rc;
    std::vector<float*> P(total, nullptr);
    for (uint32_t i = 0; i < total; ++i) {
        if ((uint32_t)T[i].storage != i) continue;
        P[i] = T[i].buf ? find_buffer(ctx->ds, T[i].buf)->dev : (float*)(ctx->arena + offs[i]);
    }
    for (uint32_t i = 0; i < total; ++i) {
        if ((uint32_t)T[i].storage != i) P[i] = P[T[i].storage] + T[i].view_off;
        ctx->last_ptr[i] = P[i];
        ctx->last_len[i] = need[T[i].storage] - T[i].view_off;
    }
    // ---- upload host leafs (token ids, rope / mask / scale parameters, caller-filled inputs)
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging buffer reuse
    uint64_t so = 0;
    for (uint32_t i = 0; i < total; ++i) {
        if ((uint32_t)T[i].storage != i || T[i].buf || !T[i].host) continue;
        const uint64_t bytes = nelem(T[i]) * 4;
        memcpy(ctx->staging + so, T[i].host, bytes);
        LH_HIP(ctx, hipMemcpyAsync(P[i], ctx->staging + so, bytes, hipMemcpyHostToDevice, ctx->stream));
        so += (bytes + 15) & ~(uint64_t)15;
    }
    // ---- sequential walk (ml.go:1501-1526)
    for (uint32_t i = n_leafs; i < total; ++i)
        if ((rc = run_node(ctx, T, P, i))) return rc;
    mark_end();
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

int lh_graph_check(const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, char* msg, uint64_t cap) {
    return gc::graph_check(T, n_leafs, n_nodes, bufs, n_bufs, msg, cap);
}

int lh_graph_match(const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, lh_match_info* out) {
    return gm::graph_match(T, n_leafs, n_nodes, bufs, n_bufs, out);
}

int lh_node_read(lh_ctx* ctx, uint32_t index, uint64_t off, float* dst, uint64_t n) {
    if (!ctx || !dst) return LH_EINVAL;
    if (index >= ctx->last_ptr.size() || !ctx->last_ptr[index])
        LH_FAIL(ctx, LH_EINVAL, "lh_node_read: tensor %u was not materialised by the last graph (a fused plan keeps the final node and the nodes flagged LH_T_OUTPUT; flag it, or use LH_GRAPH_NO_FUSION)", index);
    if (off > ctx->last_len[index] || n > ctx->last_len[index] - off) LH_FAIL(ctx, LH_EINVAL, "lh_node_read: range outside tensor %u", index);
    if ((int64_t)index == ctx->pre_index && off == ctx->pre_off && n == ctx->pre_n) {   // already on the host (lh_graph_compute synchronised behind the copy)
        memcpy(dst, ctx->out_pinned, n * 4);
        return LH_OK;
    }
    LH_HIP(ctx, hipSetDevice(ctx->device));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    LH_HIP(ctx, hipMemcpyAsync(dst, ctx->last_ptr[index] + off, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}

int lh_last_graph_fused(lh_ctx* ctx) { return ctx ? ctx->last_fused : 0; }

int lh_ctx_time_computes(lh_ctx* ctx, int on) {
    if (!ctx) return LH_EINVAL;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (on && !ctx->tc_ev0) {
        LH_HIP(ctx, hipEventCreate(&ctx->tc_ev0));
        LH_HIP(ctx, hipEventCreate(&ctx->tc_ev1));
    }
    ctx->tc_on = on != 0; ctx->tc_end = false;
    ctx->tc_calls = 0; ctx->tc_wall_us = ctx->tc_dev_us = 0;
    return LH_OK;
}
int lh_ctx_compute_stats(lh_ctx* ctx, lh_compute_stats* out) {
    if (!ctx || !out) return LH_EINVAL;
    out->calls = ctx->tc_calls; out->wall_us = ctx->tc_wall_us; out->device_us = ctx->tc_dev_us;
    return LH_OK;
}

}  // extern "C"
