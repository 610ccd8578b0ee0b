// csrc/kernels_score.h — per-row scores of a block of logits on the device: ln p(target), ln sum exp, the greedy id and the target's rank,
// so that the [n][V] logits of an all-row Eval (llama.go:384) never travel to the host (128 KB per row at V = 32000).
//
// Definition (what tests/test_gpu_score.py restates in numpy float64), per row x[0..V):
//   m = max_j x_j;  s = sum_j exp_f64((double)x_j - (double)m), accumulated in f64;  lse = m + log(s);  logprob = (double)x_t - lse
// - the f64 exp of the reference's own softmax (llama.go:581-609, ml.go:2491).  Entries equal to -inf add exp(-inf) = 0.  A NaN in the row
// makes s a NaN whatever the order of the sum; a maximum of +inf (inf - inf) or -inf (every entry -inf) gives lse = logprob = NaN as well.
//   argmax      = lowest index of the maximum (strict >, as k_argmax_advance)
//   target_rank = #{j : x_j > x_t} + #{j < t : x_j == x_t}: the target's place in the order "value descending, id ascending"
//
// One workgroup of 1024 threads per row.  k_score_rows<EPT> with EPT > 0: V <= 1024 EPT, V % 4 == 0, row 16-byte aligned.  Every thread
// loads its EPT / 4 16-byte pieces up front (piece c of thread t = ids 4 (t + 1024 c) .. +3: a wave reads 1 KB contiguous per load) and keeps
// them in registers: the row is read once.  Pass 1 over the registers: (max, lowest index) per thread, reduced over the wave with DPP inside
// the rows of 16 lanes + four lane reads, over the 16 waves through LDS.  Pass 2 over the same registers: the f64 sum and the rank
// count, reduced the same way.  k_score_rows<0>: any V and alignment - the same two passes, each reading the row from memory with
// 4-byte loads (the second read comes from L2).
// targets[row] == SCORE_TARGET_ARGMAX scores the row against its own greedy id (lh_llama_score's last row without a next token).
#pragma once
#include "kernels_common.h"
#include "../../include/llamahip.h"

namespace lh {

constexpr uint32_t SCORE_TARGET_ARGMAX = 0xFFFFFFFFu;

struct ScoreBest { float v; uint32_t i; };   // i == 0xFFFFFFFF: nothing seen yet (loses every tie)

__device__ __forceinline__ ScoreBest score_better(ScoreBest a, ScoreBest b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

template <int CTRL>
__device__ __forceinline__ uint32_t score_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ ScoreBest score_dpp_best(ScoreBest b) { return ScoreBest{__uint_as_float(score_dpp<CTRL>(__float_as_uint(b.v))), score_dpp<CTRL>(b.i)}; }
template <int CTRL>
__device__ __forceinline__ double score_dpp_f64(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return __longlong_as_double((long long)(((uint64_t)score_dpp<CTRL>((uint32_t)(u >> 32)) << 32) | score_dpp<CTRL>((uint32_t)u)));
}
__device__ __forceinline__ uint32_t score_lane_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ double score_lane_f64(double v, int l) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return __longlong_as_double((long long)(((uint64_t)score_lane_u32((uint32_t)(u >> 32), l) << 32) | score_lane_u32((uint32_t)u, l)));
}

// (max, lowest index) over the 64 lanes, uniform: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, then the four rows
__device__ __forceinline__ ScoreBest score_wave_best(ScoreBest b) {
    b = score_better(b, score_dpp_best<0xB1>(b));
    b = score_better(b, score_dpp_best<0x4E>(b));
    b = score_better(b, score_dpp_best<0x141>(b));
    b = score_better(b, score_dpp_best<0x140>(b));
    ScoreBest r = ScoreBest{__uint_as_float(score_lane_u32(__float_as_uint(b.v), 0)), score_lane_u32(b.i, 0)};
#pragma unroll
    for (int l = 16; l < 64; l += 16) r = score_better(r, ScoreBest{__uint_as_float(score_lane_u32(__float_as_uint(b.v), l)), score_lane_u32(b.i, l)});
    return r;
}
__device__ __forceinline__ double score_wave_sum_f64(double v) {   // fixed association: deterministic
    v += score_dpp_f64<0xB1>(v);
    v += score_dpp_f64<0x4E>(v);
    v += score_dpp_f64<0x141>(v);
    v += score_dpp_f64<0x140>(v);
    return (score_lane_f64(v, 0) + score_lane_f64(v, 16)) + (score_lane_f64(v, 32) + score_lane_f64(v, 48));
}
__device__ __forceinline__ uint32_t score_wave_sum_u32(uint32_t v) {
    v += score_dpp<0xB1>(v);
    v += score_dpp<0x4E>(v);
    v += score_dpp<0x141>(v);
    v += score_dpp<0x140>(v);
    return (score_lane_u32(v, 0) + score_lane_u32(v, 16)) + (score_lane_u32(v, 32) + score_lane_u32(v, 48));
}

// Two workgroups per CU where the registers allow it (8 waves per SIMD = 64 VGPRs; EPT = 64 needs 106): the loads of one row then run under the
// f64 exps of another - the exps, not the bytes, bound this kernel (profiles/score_rows.txt).
template <int EPT>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(EPT == 64 ? 4 : 8, EPT == 64 ? 4 : 8))) void k_score_rows(const float* __restrict__ logits, uint32_t V, const uint32_t* __restrict__ targets, lh_row_score* __restrict__ out) {
    __shared__ float sv[16];
    __shared__ uint32_t si[16], sc[16];
    __shared__ double ss[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t row = blockIdx.x;
    const float* __restrict__ x = logits + (size_t)row * V;
    constexpr int NP = EPT > 0 ? EPT / 4 : 1;
    f4 lv[NP];
    if constexpr (EPT > 0) {   // all loads first, unconditional (clamped): they are in flight together
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            const uint32_t i0 = 4u * ((uint32_t)tid + 1024u * (uint32_t)c);
            lv[c] = *(const f4*)(x + (i0 < V ? i0 : V - 4));
        }
    }
    uint32_t t = targets[row];
    const float xt_mem = x[t < V ? t : 0];

    // pass 1: the maximum and its lowest index (ids ascend inside a thread: the first maximum is kept)
    ScoreBest b = ScoreBest{-INFINITY, 0xFFFFFFFFu};
    auto take = [&](float v, uint32_t i) {
        if (v > b.v || b.i == 0xFFFFFFFFu) { b.v = v; b.i = i; }
    };
    if constexpr (EPT > 0) {
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            const uint32_t i0 = 4u * ((uint32_t)tid + 1024u * (uint32_t)c);
            if (i0 < V) { take(lv[c].x, i0); take(lv[c].y, i0 + 1); take(lv[c].z, i0 + 2); take(lv[c].w, i0 + 3); }
        }
    } else {
        for (uint32_t i = tid; i < V; i += 1024) take(x[i], i);
    }
    b = score_wave_best(b);
    if (lane == 0) { sv[wave] = b.v; si[wave] = b.i; }
    __syncthreads();
    b = ScoreBest{sv[0], si[0]};
#pragma unroll
    for (int w = 1; w < 16; ++w) b = score_better(b, ScoreBest{sv[w], si[w]});
    const float m = b.v;
    const float xt = t == SCORE_TARGET_ARGMAX ? m : xt_mem;
    t = t == SCORE_TARGET_ARGMAX ? b.i : t;

    // pass 2: f64 sum of exp(x - m), and how many entries come before the target in (value descending, id ascending)
    const double md = (double)m;
    double s = 0.0;
    uint32_t cnt = 0;
    auto add = [&](float v, uint32_t i) {
        s += exp((double)v - md);
        cnt += (v > xt || (v == xt && i < t)) ? 1u : 0u;
    };
    if constexpr (EPT > 0) {
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            const uint32_t i0 = 4u * ((uint32_t)tid + 1024u * (uint32_t)c);
            if (i0 < V) { add(lv[c].x, i0); add(lv[c].y, i0 + 1); add(lv[c].z, i0 + 2); add(lv[c].w, i0 + 3); }
        }
    } else {
        for (uint32_t i = tid; i < V; i += 1024) add(x[i], i);
    }
    s = score_wave_sum_f64(s);
    cnt = score_wave_sum_u32(cnt);
    if (lane == 0) { ss[wave] = s; sc[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        double st = 0.0;
        uint32_t ct = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { st += ss[w]; ct += sc[w]; }
        const bool finite_max = m == m && m != INFINITY && m != -INFINITY;
        const double lse = finite_max ? md + log(st) : __longlong_as_double(0x7FF8000000000000ll);
        lh_row_score r;
        r.logprob = (double)xt - lse;
        r.lse = lse;
        r.target_logit = xt;
        r.max_logit = m;
        r.argmax = b.i;
        r.target_rank = ct;
        out[row] = r;
    }
}

}  // namespace lh
