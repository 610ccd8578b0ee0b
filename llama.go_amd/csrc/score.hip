// csrc/score.hip — host side of the row scorer (kernels_score.h): the launch helper, the op-level entry on host logits and the scored Eval
// (llama.Eval with the lm_head of all N rows, llama.go:384, reduced on the device).
#include "plan.h"
#include "kernels_score.h"

static_assert(sizeof(lh_row_score) == 32, "lh_row_score is part of the ABI: 32 bytes");

namespace lh {

// n rows of V logits (device, row stride V) against targets (device; SCORE_TARGET_ARGMAX = the row's own greedy id) -> out[n] (device)
int score_launch(lh_ctx* ctx, const float* logits, uint32_t n, uint32_t V, const uint32_t* targets, lh_row_score* out) {
    const bool vec = (V & 3u) == 0 && ((uintptr_t)logits & 15u) == 0;   // every row 16-byte aligned
    if (vec && V <= 4u * 1024u) LH_LAUNCH(k_score_rows<4>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, targets, out);
    else if (vec && V <= 32u * 1024u) LH_LAUNCH(k_score_rows<32>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, targets, out);
    else if (vec && V <= 64u * 1024u) LH_LAUNCH(k_score_rows<64>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, targets, out);
    else LH_LAUNCH(k_score_rows<0>, dim3(n), dim3(1024), 0, ctx->stream, logits, V, targets, out);
    LH_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace lh

using namespace lh;

extern "C" int lh_score_rows(lh_ctx* ctx, const float* logits_host, uint32_t n_rows, uint32_t n_logits, const uint32_t* targets_host, lh_row_score* out_host) {
    if (!ctx) return LH_EINVAL;
    if (!logits_host || !targets_host || !out_host) LH_FAIL(ctx, LH_EINVAL, "lh_score_rows: null argument");
    if (n_rows == 0 || n_logits == 0) LH_FAIL(ctx, LH_EINVAL, "lh_score_rows: %u rows of %u logits", n_rows, n_logits);
    for (uint32_t i = 0; i < n_rows; ++i)
        if (targets_host[i] >= n_logits) LH_FAIL(ctx, LH_EINVAL, "lh_score_rows: target id %u of row %u outside the vocabulary of %u", targets_host[i], i, n_logits);
    LH_HIP(ctx, hipSetDevice(ctx->device));
    // one allocation: logits | scores | targets
    const size_t o_out = (((size_t)n_rows * n_logits * 4) + 15) & ~(size_t)15, o_tgt = o_out + (size_t)n_rows * sizeof(lh_row_score), total = o_tgt + (size_t)n_rows * 4;
    char* dev = nullptr;
    LH_HIP(ctx, hipMalloc((void**)&dev, total));
    hipError_t e = hipMemcpyAsync(dev, logits_host, (size_t)n_rows * n_logits * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + o_tgt, targets_host, (size_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's arrays are pageable host memory
    if (e == hipSuccess) {
        const int rc = score_launch(ctx, (const float*)dev, n_rows, n_logits, (const uint32_t*)(dev + o_tgt), (lh_row_score*)(dev + o_out));
        if (rc) { hipFree(dev); return rc; }
        e = hipMemcpyAsync(out_host, dev + o_out, (size_t)n_rows * sizeof(lh_row_score), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(dev);
    if (e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "lh_score_rows: %s", hipGetErrorString(e));
    return LH_OK;
}

extern "C" int lh_llama_score(lh_llama* m, const uint32_t* tokens, uint32_t n, uint32_t past, const uint32_t* targets, lh_row_score* out_host) {
    if (!m || !tokens || !out_host) return LH_EINVAL;
    lh_ctx* ctx = m->ctx;
    Plan* p = m->plan;
    const ModelDesc& md = p->md;
    LH_HIP(ctx, hipSetDevice(ctx->device));
    if (!md.last_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_score: this stage holds no lm_head (layers [%u, %u) of %u)", md.layer0, md.layer1, md.L);
    if (!md.first_stage()) LH_FAIL(ctx, LH_EUNSUPPORTED, "lh_llama_score: a last stage without the embeddings has no token input here; score on a whole-model plan");
    if (n == 0) LH_FAIL(ctx, LH_EINVAL, "lh_llama_score: empty token batch");
    if ((uint64_t)past + n > md.ctx) LH_FAIL(ctx, LH_EINVAL, "lh_llama_score: past %u + n %u exceeds the context window of %u", past, n, md.ctx);
    for (uint32_t i = 0; i < n; ++i)
        if (tokens[i] >= md.V) LH_FAIL(ctx, LH_EINVAL, "lh_llama_score: token id %u at index %u outside the vocabulary of %u", tokens[i], i, md.V);
    if (targets)
        for (uint32_t i = 0; i < n; ++i)
            if (targets[i] >= md.V) LH_FAIL(ctx, LH_EINVAL, "lh_llama_score: target id %u of row %u outside the vocabulary of %u", targets[i], i, md.V);
    if (n > p->score_cap) {
        LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (p->score_dev) LH_HIP(ctx, hipFree(p->score_dev));
        p->score_dev = nullptr;
        p->score_cap = 0;
        LH_HIP(ctx, hipMalloc((void**)&p->score_dev, (size_t)n * (sizeof(lh_row_score) + 4)));
        p->score_cap = n;
    }
    lh_row_score* out_dev = (lh_row_score*)p->score_dev;
    uint32_t* tgt_dev = (uint32_t*)(p->score_dev + (size_t)p->score_cap * sizeof(lh_row_score));
    std::vector<uint32_t> next;
    if (!targets) {   // the next token of the sequence; the last row has none: its own greedy id
        next.assign(tokens + 1, tokens + n);
        next.push_back(SCORE_TARGET_ARGMAX);
        targets = next.data();
    }
    LH_HIP(ctx, hipMemcpy(tgt_dev, targets, (size_t)n * 4, hipMemcpyHostToDevice));   // (every earlier call drained the stream: the buffer is idle)
    int rc;
    if ((rc = plan_eval(p, tokens, nullptr, nullptr, n, past, false))) return rc;
    if ((rc = score_launch(ctx, p->logits, n, md.V, tgt_dev, out_dev))) return rc;
    LH_HIP(ctx, hipMemcpyAsync(out_host, out_dev, (size_t)n * sizeof(lh_row_score), hipMemcpyDeviceToHost, ctx->stream));
    LH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LH_OK;
}
