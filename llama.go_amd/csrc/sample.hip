// csrc/sample.hip — host side of the device sampler (kernels_sample.h): parameter checks, the launch helper the resident
// decode loop uses, and a one-shot entry point for op-level parity tests on arbitrary logits.
#include "plan.h"
#include "kernels_sample.h"

namespace lh {

int sample_check(lh_ctx* ctx, const lh_sample_params* sp, uint32_t V) {
    if (!sp) LH_FAIL(ctx, LH_EINVAL, "sampler: null parameters");
    if (V == 0 || V > 64u * 1024u) LH_FAIL(ctx, LH_ESHAPE, "sampler: vocabulary of %u ids outside the supported 1..65536", V);
    // the reference slices logitsID[:topK] (llama.go:567) and panics when topK > len(logits)
    if (sp->top_k == 0 || sp->top_k > V) LH_FAIL(ctx, LH_EINVAL, "sampler: topK = %u outside 1..%u", sp->top_k, V);
    if (sp->top_k > SAMPLE_MAX_K) LH_FAIL(ctx, LH_EUNSUPPORTED, "sampler: topK = %u above the device limit of %u", sp->top_k, SAMPLE_MAX_K);
    if (!(sp->temp > 0.0f)) LH_FAIL(ctx, LH_EINVAL, "sampler: temp must be > 0 (main.go:379-381 replaces 0 by 0.5)");
    if (!(sp->repeat_penalty > 0.0f)) LH_FAIL(ctx, LH_EINVAL, "sampler: repeatPenalty must be > 0");
    return 0;
}

int sample_launch(lh_ctx* ctx, const float* logits, uint32_t V, SampleState* st, uint32_t* ring, StepParams* sp, uint32_t* out_tokens, uint32_t* token_out,
                  uint32_t* dbg_ids, float* dbg_probs, uint32_t* dbg_keep, int advance, uint32_t topk_hint) {
    const bool small_k = topk_hint && topk_hint <= 64;
    if (small_k && V <= 32u * 1024u)
        LH_LAUNCH(k_sample_small<32>, dim3(1), dim3(1024), 0, ctx->stream, logits, V, st, ring, sp, out_tokens, token_out, dbg_ids, dbg_probs, dbg_keep, advance);
    else if (small_k)
        LH_LAUNCH(k_sample_small<64>, dim3(1), dim3(1024), 0, ctx->stream, logits, V, st, ring, sp, out_tokens, token_out, dbg_ids, dbg_probs, dbg_keep, advance);
    else if (V <= 32u * 1024u)
        LH_LAUNCH(k_sample<32>, dim3(1), dim3(1024), 0, ctx->stream, logits, V, st, ring, sp, out_tokens, token_out, dbg_ids, dbg_probs, dbg_keep, advance);
    else
        LH_LAUNCH(k_sample<64>, dim3(1), dim3(1024), 0, ctx->stream, logits, V, st, ring, sp, out_tokens, token_out, dbg_ids, dbg_probs, dbg_keep, advance);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

int sample_rows_launch(lh_ctx* ctx, const float* logits, uint32_t V, uint32_t n_rows, SampleState* st, uint32_t* ring, const uint32_t* tok, const uint32_t* n_draft,
                       uint32_t* arg, uint32_t topk_hint) {
    const bool small_k = topk_hint && topk_hint <= 64;
    if (small_k && V <= 32u * 1024u)
        LH_LAUNCH(k_sample_small_rows<32>, dim3(n_rows), dim3(1024), 0, ctx->stream, logits, V, st, ring, tok, n_draft, arg);
    else if (small_k)
        LH_LAUNCH(k_sample_small_rows<64>, dim3(n_rows), dim3(1024), 0, ctx->stream, logits, V, st, ring, tok, n_draft, arg);
    else if (V <= 32u * 1024u)
        LH_LAUNCH(k_sample_rows<32>, dim3(n_rows), dim3(1024), 0, ctx->stream, logits, V, st, ring, tok, n_draft, arg);
    else
        LH_LAUNCH(k_sample_rows<64>, dim3(n_rows), dim3(1024), 0, ctx->stream, logits, V, st, ring, tok, n_draft, arg);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

int sample_pod_rows_launch(lh_ctx* ctx, const float* logits, uint32_t V, uint32_t n_pods, uint32_t n_rows, SampleState* ss, uint32_t* ring, uint32_t ring_cap,
                           const uint32_t* tok, const SpecState* st, uint32_t* arg, uint32_t topk_hint) {
    const bool small_k = topk_hint && topk_hint <= 64;
    const uint32_t n = n_pods * n_rows;
    LH_TRACE("%s/n%u", small_k ? "k_sample_small_pod_rows" : "k_sample_pod_rows", n);
    if (small_k && V <= 32u * 1024u)
        LH_LAUNCH(k_sample_small_pod_rows<32>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, tok, st, n_rows, arg);
    else if (small_k)
        LH_LAUNCH(k_sample_small_pod_rows<64>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, tok, st, n_rows, arg);
    else if (V <= 32u * 1024u)
        LH_LAUNCH(k_sample_pod_rows<32>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, tok, st, n_rows, arg);
    else
        LH_LAUNCH(k_sample_pod_rows<64>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, tok, st, n_rows, arg);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

int sample_pods_launch(lh_ctx* ctx, const float* logits, uint32_t V, uint32_t n_jobs, const SampleJob* jobs, SampleState* ss, uint32_t* ring, uint32_t ring_cap,
                       StepParams* sp, uint32_t* out, uint32_t out_cap, uint32_t* ids, uint32_t topk_hint) {
    const bool small_k = topk_hint && topk_hint <= 64;
    LH_TRACE("%s/n%u", small_k ? "k_sample_small_pods" : "k_sample_pods", n_jobs);
    if (small_k && V <= 32u * 1024u)
        LH_LAUNCH(k_sample_small_pods<32>, dim3(n_jobs), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, sp, out, out_cap, ids, jobs);
    else if (small_k)
        LH_LAUNCH(k_sample_small_pods<64>, dim3(n_jobs), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, sp, out, out_cap, ids, jobs);
    else if (V <= 32u * 1024u)
        LH_LAUNCH(k_sample_pods<32>, dim3(n_jobs), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, sp, out, out_cap, ids, jobs);
    else
        LH_LAUNCH(k_sample_pods<64>, dim3(n_jobs), dim3(1024), 0, ctx->stream, logits, V, ss, ring, ring_cap, sp, out, out_cap, ids, jobs);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

int feed_ring_launch(lh_ctx* ctx, const FeedRingSeg* segs, uint32_t n_segs, const uint32_t* tok, SampleState* ss, uint32_t* ring, uint32_t ring_cap) {
    LH_LAUNCH(k_feed_ring, dim3(n_segs), dim3(256), 0, ctx->stream, segs, tok, ss, ring, ring_cap);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace lh

using namespace lh;

extern "C" int lh_sample_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_rows, uint32_t n_logits, const uint32_t* ring_host, uint32_t ring_size, uint32_t ring_pos,
                              const uint32_t* tokens_host, const lh_sample_params* sp, uint64_t draw0, uint32_t* ids_out) {
    if (!ctx) return LH_EINVAL;
    if (!logits_host || !ring_host || !tokens_host || !ids_out) LH_FAIL(ctx, LH_EINVAL, "lh_sample_rows: null argument");
    if (n_rows == 0 || n_rows > 8) LH_FAIL(ctx, LH_EINVAL, "lh_sample_rows: %u rows outside 1..8", n_rows);
    if (ring_size == 0) LH_FAIL(ctx, LH_EINVAL, "lh_sample_rows: the lastNTokens ring needs at least one slot");
    int rc;
    if ((rc = sample_check(ctx, sp, n_logits))) return rc;
    for (uint32_t r = 1; r < n_rows; ++r)
        if (tokens_host[r] >= n_logits) LH_FAIL(ctx, LH_EINVAL, "lh_sample_rows: draft id %u at index %u outside the vocabulary of %u", tokens_host[r], r, n_logits);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: logits | ring | state | tokens | ids
    const size_t o_ring = (size_t)n_rows * n_logits * 4, o_st = (o_ring + (size_t)ring_size * 4 + 15) & ~(size_t)15, o_tok = o_st + sizeof(SampleState), o_ids = o_tok + 4 * 8,
                 total = o_ids + 4 * 8;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    SampleState st = {sp->top_k, sp->top_p, sp->temp, sp->repeat_penalty, sp->seed, draw0, ring_size, ring_pos};
    uint32_t ids[8] = {};
    hipError_t e = hipMemcpyAsync(dev, logits_host, o_ring, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_ring, ring_host, (size_t)ring_size * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_st, &st, sizeof st, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_tok, tokens_host, (size_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // st and the caller's arrays are pageable host memory
    if (e == hipSuccess) {
        rc = sample_rows_launch(ctx, (const float*)dev, n_logits, n_rows, (SampleState*)(dev + o_st), (uint32_t*)(dev + o_ring), (const uint32_t*)(dev + o_tok), nullptr,
                                (uint32_t*)(dev + o_ids), sp->top_k);
        if (rc) { hipFree(dev); return rc; }
        e = hipMemcpyAsync(ids, dev + o_ids, (size_t)n_rows * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_sample_rows: %s", hipGetErrorString(e));
    for (uint32_t r = 0; r < n_rows; ++r) ids_out[r] = ids[r];
    return LH_OK;
}

extern "C" int lh_sample_top_p_top_k(lh_ctx* ctx, const float* logits, uint32_t n_logits, const uint32_t* last_n_tokens, uint32_t n_last, const lh_sample_params* sp,
                                     uint64_t draw, uint32_t* token_out, uint32_t* cand_ids, float* cand_probs, uint32_t* n_keep) {
    if (!ctx) return LH_EINVAL;
    if (!logits || !token_out || (n_last && !last_n_tokens)) LH_FAIL(ctx, LH_EINVAL, "lh_sample_top_p_top_k: null argument");
    int rc;
    if ((rc = sample_check(ctx, sp, n_logits))) return rc;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: logits | ring | state | token, keep | ids | probs
    const size_t o_ring = (size_t)n_logits * 4, o_st = o_ring + (size_t)(n_last ? n_last : 1) * 4, o_tok = o_st + sizeof(SampleState), o_ids = o_tok + 8,
                 o_pr = o_ids + (size_t)sp->top_k * 4, total = o_pr + (size_t)sp->top_k * 4;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    SampleState st = {sp->top_k, sp->top_p, sp->temp, sp->repeat_penalty, sp->seed, draw, n_last, 0};
    hipError_t e = hipMemcpyAsync(dev, logits, (size_t)n_logits * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n_last) e = hipMemcpyAsync(dev + o_ring, last_n_tokens, (size_t)n_last * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_st, &st, sizeof st, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // st and the caller's arrays are pageable host memory
    if (e == hipSuccess) {
        rc = sample_launch(ctx, (const float*)dev, n_logits, (SampleState*)(dev + o_st), (uint32_t*)(dev + o_ring), nullptr, nullptr, (uint32_t*)(dev + o_tok),
                           (uint32_t*)(dev + o_ids), (float*)(dev + o_pr), (uint32_t*)(dev + o_tok + 4), 0, sp->top_k);
        if (rc) { hipFree(dev); return rc; }
        uint32_t tk[2] = {0, 0};
        e = hipMemcpyAsync(tk, dev + o_tok, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) {
            *token_out = tk[0];
            if (n_keep) *n_keep = tk[1];
            if (cand_ids) e = hipMemcpy(cand_ids, dev + o_ids, (size_t)tk[1] * 4, hipMemcpyDeviceToHost);
            if (e == hipSuccess && cand_probs) e = hipMemcpy(cand_probs, dev + o_pr, (size_t)tk[1] * 4, hipMemcpyDeviceToHost);
        }
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_sample_top_p_top_k: %s", hipGetErrorString(e));
    return LH_OK;
}

extern "C" int lh_sample_pods(lh_ctx* ctx, const float* logits_host, uint32_t n, uint32_t n_logits, const uint32_t* rings_host, uint32_t ring_size,
                              const uint32_t* ring_pos, const uint64_t* draws, const lh_sample_params* sp, uint32_t* ids_out, uint32_t* rings_out,
                              uint32_t* ring_pos_out) {
    if (!ctx) return LH_EINVAL;
    if (!logits_host || !rings_host || !ring_pos || !draws || !ids_out) LH_FAIL(ctx, LH_EINVAL, "lh_sample_pods: null argument");
    if (n == 0 || n > 64) LH_FAIL(ctx, LH_EINVAL, "lh_sample_pods: %u pods outside 1..64", n);
    if (ring_size == 0) LH_FAIL(ctx, LH_EINVAL, "lh_sample_pods: the lastNTokens ring needs at least one slot");
    int rc;
    if ((rc = sample_check(ctx, sp, n_logits))) return rc;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: logits | rings | states | step parameters | output lists (one entry each) | ids
    const size_t b_lg = (size_t)n * n_logits * 4, b_ring = (size_t)n * ring_size * 4;
    const size_t o_ring = b_lg, o_st = (o_ring + b_ring + 15) & ~(size_t)15, o_sp = o_st + sizeof(SampleState) * 64, o_out = o_sp + sizeof(StepParams) * 64,
                 o_ids = o_out + 4 * 64, total = o_ids + 4 * 64;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    SampleState st[64];
    for (uint32_t i = 0; i < n; ++i) st[i] = SampleState{sp->top_k, sp->top_p, sp->temp, sp->repeat_penalty, sp->seed, draws[i], ring_size, ring_pos[i]};
    uint32_t ids[64] = {};
    hipError_t e = hipMemcpyAsync(dev, logits_host, b_lg, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_ring, rings_host, b_ring, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_st, st, sizeof(SampleState) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dev + o_sp, 0, o_ids - o_sp, ctx->stream);   // step 0 of a one-entry output list per pod
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // st and the caller's arrays are pageable host memory
    if (e == hipSuccess) {
        rc = sample_pods_launch(ctx, (const float*)dev, n_logits, n, nullptr, (SampleState*)(dev + o_st), (uint32_t*)(dev + o_ring), ring_size, (StepParams*)(dev + o_sp),
                                (uint32_t*)(dev + o_out), 1, (uint32_t*)(dev + o_ids), sp->top_k);
        if (rc) { hipFree(dev); return rc; }
        e = hipMemcpyAsync(ids, dev + o_ids, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && rings_out) e = hipMemcpyAsync(rings_out, dev + o_ring, b_ring, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && ring_pos_out) e = hipMemcpyAsync(st, dev + o_st, sizeof(SampleState) * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_sample_pods: %s", hipGetErrorString(e));
    for (uint32_t i = 0; i < n; ++i) {
        ids_out[i] = ids[i];
        if (ring_pos_out) ring_pos_out[i] = st[i].ring_pos;
    }
    return LH_OK;
}

extern "C" int lh_sample_pod_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_pods, uint32_t n_rows, uint32_t n_logits, const uint32_t* rings_host,
                                  uint32_t ring_size, const uint32_t* ring_pos, const uint64_t* draws, const uint32_t* tokens_host, const uint32_t* n_draft,
                                  const lh_sample_params* sp, uint32_t* ids_out) {
    if (!ctx) return LH_EINVAL;
    if (!logits_host || !rings_host || !ring_pos || !draws || !tokens_host || !n_draft || !ids_out) LH_FAIL(ctx, LH_EINVAL, "lh_sample_pod_rows: null argument");
    const uint32_t P = n_pods, R = n_rows;
    if (P == 0 || P > 64 || R == 0 || R > 8 || P * R > 64)
        LH_FAIL(ctx, LH_EINVAL, "lh_sample_pod_rows: %u pods x %u rows (1..64 pods, 1..8 rows, at most 64 rows in all)", P, R);
    if (ring_size == 0) LH_FAIL(ctx, LH_EINVAL, "lh_sample_pod_rows: the lastNTokens ring needs at least one slot");
    int rc;
    if ((rc = sample_check(ctx, sp, n_logits))) return rc;
    for (uint32_t i = 0; i < P; ++i)
        for (uint32_t r = 1; r < R; ++r)
            if (tokens_host[(size_t)i * R + r] >= n_logits)
                LH_FAIL(ctx, LH_EINVAL, "lh_sample_pod_rows: pod %u: draft id %u at index %u outside the vocabulary of %u", i, tokens_host[(size_t)i * R + r], r, n_logits);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: logits | rings | sampler states | pass states (k = n_draft, one id asked for, none produced) | tokens | ids
    const size_t n = (size_t)P * R, b_lg = n * n_logits * 4, b_ring = (size_t)P * ring_size * 4;
    const size_t o_ring = b_lg, o_st = (o_ring + b_ring + 63) & ~(size_t)63, o_ps = o_st + sizeof(SampleState) * 64, o_tok = o_ps + sizeof(SpecState) * 64, o_ids = o_tok + 4 * 64,
                 total = o_ids + 4 * 64;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    SampleState st[64];
    SpecState ps[64] = {};
    for (uint32_t i = 0; i < P; ++i) {
        st[i] = SampleState{sp->top_k, sp->top_p, sp->temp, sp->repeat_penalty, sp->seed, draws[i], ring_size, ring_pos[i]};
        ps[i].n_steps = 1; ps[i].k = n_draft[i];
    }
    uint32_t ids[64];
    hipError_t e = hipMemcpyAsync(dev, logits_host, b_lg, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_ring, rings_host, b_ring, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_st, st, sizeof(SampleState) * P, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_ps, ps, sizeof(SpecState) * P, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_tok, tokens_host, n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dev + o_ids, 0xFF, 4 * 64, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the host arrays are pageable memory
    if (e == hipSuccess) {
        rc = sample_pod_rows_launch(ctx, (const float*)dev, n_logits, P, R, (SampleState*)(dev + o_st), (uint32_t*)(dev + o_ring), ring_size, (const uint32_t*)(dev + o_tok),
                                    (const SpecState*)(dev + o_ps), (uint32_t*)(dev + o_ids), sp->top_k);
        if (rc) { (void)hipFree(dev); return rc; }
        e = hipMemcpyAsync(ids, dev + o_ids, n * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_sample_pod_rows: %s", hipGetErrorString(e));
    for (uint32_t i = 0; i < P; ++i)
        for (uint32_t r = 0; r < R && r <= n_draft[i]; ++r) ids_out[(size_t)i * R + r] = ids[(size_t)i * R + r];   // the rows behind a draft stay the caller's
    return LH_OK;
}
