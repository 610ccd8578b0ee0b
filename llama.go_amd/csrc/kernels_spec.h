// csrc/kernels_spec.h — lookup-draft speculative decoding (greedy and sampled, lossless): the n-gram drafter and the accept step on the device.
// A pass evaluates [pending, d1..dk] (+ filler rows up to a fixed row count) as one multi-row pass of the stream's own cache (kernels_rows.h:
// every row bit-identical to its solo one-token step); k_batch_argmax takes the rows' greedy ids (sampled route: k_sample_rows the rows' sampled ids); k_spec_accept keeps the longest prefix of the
// draft the model itself produced, moves the row table on by the accepted count and drafts for the next pass.  The rule is stated in
// include/llamahip.h (lh_lookup_params) and restated in tests/speculative_ref.py.
#pragma once
#include "kernels_common.h"
#include "kernels_sample.h"

namespace lh {

constexpr uint32_t SPEC_UNKNOWN = 0xFFFFFFFFu;   // = Plan::HIST_UNKNOWN: a window entry the context does not know
constexpr int SPEC_TH = 1024;
constexpr uint32_t SPEC_ROWS_MAX = 8, SPEC_NGRAM_MAX = 8, SPEC_CORPUS_MAX = 65536;

// (SpecState, the loop's state in device memory, is defined in kernels_sample.h: the pods x rows sampler reads it.)
struct SpecLookup {
    const uint32_t* corpus;   // device, may be nullptr
    uint32_t n_corpus, draft_max, ngram_max, ngram_min;
};
struct SpecToks { uint32_t t[SPEC_ROWS_MAX]; };

// The largest j in [0, n_j) with src[j..j+G) == S, or -1: every thread walks its j ascending (its last hit is its largest), one LDS max over the block.
// Called by all threads of the block; the result is uniform.
__device__ __forceinline__ int spec_find_last(const uint32_t* __restrict__ src, uint32_t n_j, uint32_t G, const uint32_t (&S)[SPEC_NGRAM_MAX], int* s_best) {
    __syncthreads();   // (the readers of the previous search are done)
    if (threadIdx.x == 0) *s_best = -1;
    __syncthreads();
    int best = -1;
    for (uint32_t j = threadIdx.x; j < n_j; j += SPEC_TH) {
        bool eq = src[j] == S[0];
#pragma unroll
        for (uint32_t g = 1; g < SPEC_NGRAM_MAX; ++g)
            if (eq && g < G) eq = src[j + g] == S[g];
        if (eq) best = (int)j;
    }
    if (best >= 0) atomicMax(s_best, best);
    __syncthreads();
    return *s_best;
}

// The draft rule (include/llamahip.h) over the window H[0..n) (H[n-1] = the pending token) and the corpus: up to min(draft_max, limit) ids into dst,
// the count returned (uniform).  An id >= vocab in a continuation (an unknown window entry) ends the draft in front of it.
__device__ __forceinline__ uint32_t spec_lookup(const uint32_t* __restrict__ H, uint32_t n, const SpecLookup lp, uint32_t limit, uint32_t vocab,
                                                uint32_t* __restrict__ dst, int* s_best) {
    uint32_t K = lp.draft_max < limit ? lp.draft_max : limit;
    if (K > SPEC_ROWS_MAX - 1) K = SPEC_ROWS_MAX - 1;
    if (K == 0 || n == 0) return 0;
    for (uint32_t G = lp.ngram_max; G >= lp.ngram_min && G >= 1; --G) {
        if (n < G) continue;
        uint32_t S[SPEC_NGRAM_MAX];
        bool unknown = false;
#pragma unroll
        for (uint32_t g = 0; g < SPEC_NGRAM_MAX; ++g) {
            S[g] = g < G ? H[n - G + g] : 0u;
            unknown = unknown || (g < G && S[g] == SPEC_UNKNOWN);
        }
        if (unknown) continue;
        const uint32_t* src = H;
        uint32_t end = n;
        int j = n > G ? spec_find_last(H, n - G, G, S, s_best) : -1;                      // j <= n - G - 1: the suffix may not match itself
        if (j < 0) {
            if (!lp.corpus || lp.n_corpus <= G) continue;
            j = spec_find_last(lp.corpus, lp.n_corpus - G, G, S, s_best);                 // j + G < n_corpus: at least one id follows
            if (j < 0) continue;
            src = lp.corpus; end = lp.n_corpus;
        }
        const uint32_t start = (uint32_t)j + G;
        uint32_t len = end - start;
        if (len > K) len = K;
        uint32_t k = 0;
        while (k < len && src[start + k] < vocab) ++k;   // (every thread reads the same <= 7 words)
        if (threadIdx.x < k) dst[threadIdx.x] = src[start + threadIdx.x];
        return k;
    }
    return 0;
}

// limit of the pass that starts with the pending token at position pos: it never leaves the window and never produces more ids than asked
__device__ __forceinline__ uint32_t spec_limit(uint32_t pos, uint32_t produced, uint32_t n_steps, uint32_t ctx) {
    const uint32_t n = pos + 1;
    if (n >= ctx || produced >= n_steps) return 0;
    const uint32_t a = ctx - n, b = n_steps - produced - 1;
    return a < b ? a : b;
}

// The drafter as a launch of its own.  st == nullptr: the op-level twin (lh_draft_lookup) - window, n and limit from the arguments, the count to *k_out.
// st != nullptr: the first draft of a loop - the window is win[0..st->pos], the limit the loop's; ids into tok[1..], the rows behind them get the pending
// token as filler, the count into st->k.
__global__ __launch_bounds__(SPEC_TH) void k_draft_lookup(const uint32_t* __restrict__ win, uint32_t n, const SpecLookup lp, uint32_t limit, uint32_t vocab,
                                                          uint32_t* __restrict__ dst, uint32_t* __restrict__ k_out, SpecState* st, uint32_t ctx, uint32_t n_rows) {
    __shared__ int s_best;
    if (st) {
        n = st->pos + 1;
        limit = spec_limit(st->pos, st->produced, st->n_steps, ctx);
        if (n > ctx + 1) { n = 0; limit = 0; }
    }
    const uint32_t k = spec_lookup(win, n, lp, limit, vocab, st ? dst + 1 : dst, &s_best);
    if (st) {
        const uint32_t r = threadIdx.x;
        if (r > k && r < n_rows) dst[r] = dst[0];
        if (r == 0) st->k = k;
    } else if (threadIdx.x == 0) {
        *k_out = k;
    }
}

// State, row table and tokens of the next pass from kernel arguments (stream-ordered, nothing on the host to keep alive).  reset: the counters restart.
__global__ void k_spec_set(SpecState* st, BatchRow* rows, uint32_t* tok, StepParams* sp, float* kc, float* vc, uint32_t pos, uint32_t produced, uint32_t n_steps,
                           const SpecToks toks, uint32_t k, uint32_t n_rows, uint32_t ctx, int reset) {
    const uint32_t r = threadIdx.x;
    if (r < n_rows && r < SPEC_ROWS_MAX) {
        const uint32_t q = pos + r;
        rows[r].kc = kc; rows[r].vc = vc; rows[r].pos = q < ctx ? q : ctx - 1; rows[r].step = 0;
        tok[r] = toks.t[r];
    }
    if (r == 0) {
        st->pos = pos; st->produced = produced; st->n_steps = n_steps; st->k = k; st->last_a = 0;
        if (reset) { st->passes = 0; st->drafted = 0; st->accepted = 0; st->empty = 0; }
        sp->token = toks.t[0]; sp->past = pos < ctx ? pos : ctx - 1; sp->step = 0; sp->pad = 0;
    }
}

// The accept step behind a pass of R rows whose greedy ids are arg[0..R): a = the leading i < min(k, R - 1) with arg[i] == tok[i + 1] (a filler row never
// counts); ids arg[0..a] go to the output list and the window; arg[a] is the next pending token; the table's n_rows positions become p + a + 1 ..;
// counters and trace; then (lookup_next) the draft of the next pass.  One workgroup.  Every index it writes is clamped to its buffer: the host never
// launches a pass that needs the clamp, and a mistake there must not write outside the cache or the lists.
// ss != nullptr: the sampled route - arg[] are the ids of k_sample_rows / k_sample_small_rows (row i sampled as call ss->draw + i over the ring behind
// tok[1..i]), so arg[0..a] are the ids of a + 1 consecutive one-token sampling calls; they are appended to the ring in order and ring_pos and draw
// move on by a + 1.  ss == nullptr: the greedy route, nothing of this.
__global__ __launch_bounds__(SPEC_TH) void k_spec_accept(const uint32_t* __restrict__ arg, uint32_t R, SpecState* st, BatchRow* rows, uint32_t* tok, StepParams* sp,
                                                         uint32_t* __restrict__ win, uint32_t ctx, uint32_t vocab, uint32_t* __restrict__ out,
                                                         uint16_t* __restrict__ trace, uint32_t trace_cap, const SpecLookup lp, uint32_t n_rows, int lookup_next,
                                                         SampleState* ss, uint32_t* __restrict__ ring) {
    __shared__ int s_best;
    __shared__ uint32_t s_pos, s_done;
    if (threadIdx.x == 0) {
        const uint32_t p = st->pos, produced = st->produced, n_steps = st->n_steps;
        s_done = 1; s_pos = p;
        if (produced < n_steps && p < ctx && R >= 1) {
            uint32_t k = st->k;
            if (k > R - 1) k = R - 1;
            uint32_t a = 0;
            while (a < k && arg[a] == tok[a + 1]) ++a;
            if (a > n_steps - produced - 1) a = n_steps - produced - 1;
            if (a > ctx - 1 - p) a = ctx - 1 - p;
            for (uint32_t i = 0; i <= a; ++i) { out[produced + i] = arg[i]; win[p + 1 + i] = arg[i]; }   // win has ctx + 1 entries
            if (ss) {
                const uint32_t rs = ss->ring_size, rp = ss->ring_pos;
                if (rs) for (uint32_t i = 0; i <= a; ++i) ring[(rp + i) % rs] = arg[i];   // appendToken (server.go:205) per accepted id, in order
                ss->ring_pos = rp + a + 1; ss->draw += a + 1;
            }
            const uint32_t s = st->passes;
            if (trace && s < trace_cap) trace[s] = (uint16_t)((k << 8) | a);
            st->passes = s + 1; st->drafted += k; st->accepted += a; st->empty += k == 0 ? 1u : 0u;
            st->last_a = a; st->produced = produced + a + 1;
            const uint32_t np = p + a + 1;
            st->pos = np;
            tok[0] = arg[a];
            sp->token = arg[a]; sp->past = np < ctx ? np : ctx - 1;
            s_pos = np; s_done = produced + a + 1 >= n_steps ? 1u : 0u;
        }
    }
    __syncthreads();
    const uint32_t np = s_pos;
    if (threadIdx.x < n_rows && threadIdx.x < SPEC_ROWS_MAX) {
        const uint32_t q = np + threadIdx.x;
        rows[threadIdx.x].pos = q < ctx ? q : ctx - 1;
    }
    if (!lookup_next) return;
    uint32_t k = 0;
    if (!s_done) k = spec_lookup(win, np + 1, lp, spec_limit(np, st->produced, st->n_steps, ctx), vocab, tok + 1, &s_best);
    const uint32_t r = threadIdx.x;
    if (r > k && r < n_rows && r < SPEC_ROWS_MAX) tok[r] = tok[0];
    if (r == 0) st->k = k;
}

// ---- a second model drafts (lh_llama_decode_draft; the rule is stated in include/llamahip.h) ----
// In front of the draft model's one-token steps of a pass of n rows (n <= the table's n_table rows): the draft plan's step parameters become
// {the pending token, its position, step 0}; st->k = min(n - 1, the loop's limit over ctx = min(target window, draft window)); tok[1..n_table) get
// the pending token, so every row the draft's steps do not write holds a valid id (filler).  The steps then write their ids into tok[1..n) through
// k_argmax_advance's argmax_out; entries behind k are filler too and never count (k_spec_accept reads st->k).  The host never enqueues a pass whose
// pending token stands outside the window.  Should it: the pass must not go through unnoticed, so the loop is ended in the state - n_steps = 0 makes
// k_spec_accept commit nothing, and the host's look behind the pass fails with "inconsistent state".  The draft's steps still run (the launches are
// already enqueued) and need rows inside the cache, so they get the last n; the call that did this returns an error.
__global__ void k_draft_model_begin(SpecState* st, uint32_t* __restrict__ tok, StepParams* __restrict__ draft_sp, uint32_t n, uint32_t n_table, uint32_t ctx) {
    const uint32_t r = threadIdx.x;
    const uint32_t pending = tok[0], pos = st->pos;
    if (r >= 1 && r < n_table && r < SPEC_ROWS_MAX) tok[r] = pending;
    if (r == 0) {
        const bool inside = pos < ctx && pos + n <= ctx;        // every row of this pass, on both caches
        if (!inside) st->n_steps = 0;
        const uint32_t limit = inside ? spec_limit(pos, st->produced, st->n_steps, ctx) : 0;
        st->k = n ? (n - 1 < limit ? n - 1 : limit) : 0;
        draft_sp->token = pending; draft_sp->past = inside ? pos : (ctx - n < ctx ? ctx - n : 0); draft_sp->step = 0; draft_sp->pad = 0;
    }
}

// ---- the pods of a batch (lh_batch_decode_lookup): pod i owns rows [i * R, (i + 1) * R) of the pass's table, state st[i] and window win[i][ctx + 1] ----
// What the host reads between runs of passes: 16 bytes per pod.
struct SpecPodSum { uint32_t pos, produced, passes, last_a; };
struct SpecPodsArgs {
    const uint32_t* arg;      // [P * R] greedy ids of the pass's rows
    SpecState* st;            // [P]
    BatchRow* rows;           // [P * R]
    uint32_t* tok;            // [P * R] per pod: pending, draft, filler
    uint32_t* win;            // [P][ctx + 1]; nullptr (op-level twin): no window is kept
    uint32_t* out;            // [P][out_cap] output lists
    uint16_t* trace;          // [P][trace_cap], may be nullptr
    const float* logits;      // [P * R][vocab] of the pass, may be nullptr
    float* last;              // [P][vocab]: the logits behind each pod's last id, may be nullptr
    uint32_t* pend;           // [P] the pods' pending ids (the batch's token array), may be nullptr
    uint32_t* ids;            // [P] the same (the batch's array of produced ids), may be nullptr
    SpecPodSum* sum;          // [P]
    uint32_t R, ctx, vocab, out_cap, trace_cap;
    SampleState* ss;          // [P] the sampled route (arg = the ids of k_sample_pod_rows / k_sample_small_pod_rows); nullptr: greedy
    uint32_t* ring;           // [P][ring_cap] the pods' lastNTokens rings
    uint32_t ring_cap;
};
struct SpecPodsSet { uint32_t pos[64]; uint32_t tok[64]; };

// State, table rows and tokens of every pod from kernel arguments; the caches come from the batch's own row table.  One workgroup per pod.
__global__ void k_spec_set_pods(const SpecPodsArgs A, const BatchRow* __restrict__ pods, const SpecPodsSet v, uint32_t n_steps) {
    const uint32_t i = blockIdx.x, r = threadIdx.x, pos = v.pos[i];
    if (r < A.R) {
        const uint32_t q = pos + r;
        BatchRow* row = A.rows + (size_t)i * A.R + r;
        row->kc = pods[i].kc; row->vc = pods[i].vc; row->pos = q < A.ctx ? q : A.ctx - 1; row->step = 0;
        A.tok[(size_t)i * A.R + r] = v.tok[i];
    }
    if (r == 0) {
        SpecState* st = A.st + i;
        st->pos = pos; st->produced = 0; st->n_steps = n_steps; st->k = 0; st->last_a = 0;
        st->passes = 0; st->drafted = 0; st->accepted = 0; st->empty = 0;
        A.sum[i] = SpecPodSum{pos, 0u, 0u, 0u};
    }
}

// The first draft of every pod: the rule over win[i][0..pos_i], ids into the pod's rows 1.., the pending token as filler behind them.
__global__ __launch_bounds__(SPEC_TH) void k_draft_lookup_pods(const SpecPodsArgs A, const SpecLookup lp) {
    __shared__ int s_best;
    const uint32_t i = blockIdx.x;
    SpecState* st = A.st + i;
    uint32_t* tok = A.tok + (size_t)i * A.R;
    uint32_t n = st->pos + 1, limit = spec_limit(st->pos, st->produced, st->n_steps, A.ctx);
    if (n > A.ctx + 1) { n = 0; limit = 0; }
    const uint32_t k = spec_lookup(A.win + (size_t)i * (A.ctx + 1), n, lp, limit, A.vocab, tok + 1, &s_best);
    const uint32_t r = threadIdx.x;
    if (r > k && r < A.R) tok[r] = tok[0];
    if (r == 0) st->k = k;
}

// k_spec_accept for every pod of a pass, one workgroup per pod: the same accept rule over the pod's R ids, its output list, window, counters and trace.
// A pod that still needs ids moves its R table rows and its pending token on and (lookup_next) drafts its next pass.  A pod that FINISHES in this pass
// copies logits row a (the logits behind its last id) to last[i] and leaves its table rows and tokens where they are: as filler of the later passes they
// re-evaluate the same tokens at the same positions, so no row ever stands past the window.  A finished pod changes nothing.  Every index written is
// clamped to its buffer, as in k_spec_accept.
// A.ss != nullptr: the sampled route (lh_batch_decode_sample_lookup) - arg[] are the ids of k_sample_pod_rows / k_sample_small_pod_rows, and a pod that
// accepts a appends arg[0..a] to ITS ring in order, ring_pos and draw move on by a + 1 (k_spec_accept's commit per pod).  nullptr: the greedy route.
__global__ __launch_bounds__(SPEC_TH) void k_spec_accept_pods(const SpecPodsArgs A, const SpecLookup lp, int lookup_next) {
    __shared__ int s_best;
    __shared__ uint32_t s_pos, s_done, s_fin, s_a;
    const uint32_t i = blockIdx.x, R = A.R;
    SpecState* st = A.st + i;
    const uint32_t* arg = A.arg + (size_t)i * R;
    uint32_t* tok = A.tok + (size_t)i * R;
    uint32_t* win = A.win ? A.win + (size_t)i * (A.ctx + 1) : nullptr;
    if (threadIdx.x == 0) {
        const uint32_t p = st->pos, produced = st->produced, n_steps = st->n_steps;
        s_done = 1; s_fin = 0; s_a = 0; s_pos = p;
        if (produced < n_steps && p < A.ctx && R >= 1) {
            uint32_t k = st->k;
            if (k > R - 1) k = R - 1;
            uint32_t a = 0;
            while (a < k && arg[a] == tok[a + 1]) ++a;
            if (a > n_steps - produced - 1) a = n_steps - produced - 1;
            if (a > A.ctx - 1 - p) a = A.ctx - 1 - p;
            for (uint32_t j = 0; j <= a; ++j) {
                if (produced + j < A.out_cap) A.out[(size_t)i * A.out_cap + produced + j] = arg[j];
                if (win) win[p + 1 + j] = arg[j];   // win has ctx + 1 entries
            }
            if (A.ss) {   // the sampled commit of k_spec_accept, on the pod's own state and ring
                SampleState* ss = A.ss + i;
                uint32_t* ring = A.ring + (size_t)i * A.ring_cap;
                const uint32_t rs = ss->ring_size, rp = ss->ring_pos;
                if (rs) for (uint32_t j = 0; j <= a; ++j) ring[(rp + j) % rs] = arg[j];   // appendToken (server.go:205) per accepted id, in order
                ss->ring_pos = rp + a + 1; ss->draw += a + 1;
            }
            const uint32_t s = st->passes;
            if (A.trace && s < A.trace_cap) A.trace[(size_t)i * A.trace_cap + s] = (uint16_t)((k << 8) | a);
            st->passes = s + 1; st->drafted += k; st->accepted += a; st->empty += k == 0 ? 1u : 0u;
            st->last_a = a; st->produced = produced + a + 1;
            const uint32_t np = p + a + 1;
            st->pos = np;
            if (A.pend) A.pend[i] = arg[a];
            if (A.ids) A.ids[i] = arg[a];
            const bool fin = produced + a + 1 >= n_steps;
            if (!fin) tok[0] = arg[a];
            s_pos = np; s_a = a; s_done = fin ? 1u : 0u; s_fin = fin ? 1u : 0u;
        }
    }
    __syncthreads();
    const uint32_t np = s_pos;
    if (s_fin && A.logits && A.last) {
        const float* src = A.logits + ((size_t)i * R + s_a) * A.vocab;
        float* dst = A.last + (size_t)i * A.vocab;
        for (uint32_t j = threadIdx.x; j < A.vocab; j += SPEC_TH) dst[j] = src[j];
    }
    if (!s_done && threadIdx.x < R) {
        const uint32_t q = np + threadIdx.x;
        A.rows[(size_t)i * R + threadIdx.x].pos = q < A.ctx ? q : A.ctx - 1;
    }
    uint32_t k = 0;
    if (lookup_next && !s_done && win) k = spec_lookup(win, np + 1, lp, spec_limit(np, st->produced, st->n_steps, A.ctx), A.vocab, tok + 1, &s_best);
    const uint32_t r = threadIdx.x;
    if (lookup_next && !s_done && r > k && r < R) tok[r] = tok[0];
    if (r == 0) {
        if (lookup_next && !s_done) st->k = k;
        A.sum[i] = SpecPodSum{st->pos, st->produced, st->passes, st->last_a};
    }
}

}  // namespace lh
