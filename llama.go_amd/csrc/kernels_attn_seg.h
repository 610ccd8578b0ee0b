// csrc/kernels_attn_seg.h — segment attention of lh_batch_feed: the two per-row decode kernels (k_attention, k_attention_split in kernels_llama.h)
// generalised to a BLOCK of up to QB query rows that share one KV cache (consecutive rows of one pod in a pass: a causal prompt chunk, or a decode row).
// The per-row kernels read a pod's K / V once per query row; here every K row and every V row of the block's key range is loaded ONCE and used for all
// QB queries (queries in registers: QB float4 per lane at hd = 128), each row masked at its own position.
// HARD REQUIREMENT: per query row the operations and their order are those of the per-row kernel for a row of the same T - the three softmax branches
// (T <= 64 / <= 128 / longer), the key-phase order of the PV sums, the chunk-local statistics of the split kernel - so the output is BIT-identical to the
// per-row kernels on the same row table (tests/test_gpu_batch_feed.py compares them byte for byte; LLAMAHIP_FEED_ROW_ATTN=1 is the switch).
// What differs is only WHO computes: the short-row softmax of row i runs on wave i (a wave-level maximum / sum has the same lane -> key mapping whichever
// wave takes it), and scores / PV terms of keys beyond a row's own length are computed for the block's longest row and dropped for the others.
#pragma once
#include "kernels_llama.h"

namespace lh {

struct AttnBlock { uint32_t row0, n; };   // rows [row0, row0 + n) of the pass's row table, n <= QB, all of one cache (layout of lh_feed_block)

// Single pass (plans without split partials: ctx <= 256, or head sizes the split kernel is not built for).  grid = (H, blocks), 1024 threads.
// Dynamic LDS: sc[QB][Tp] | pr[QB][Tp] | scratch[QB][ATT_TH]; Tp = the pass's longest key range rounded up to 64.
template <int QB>
__global__ __launch_bounds__(ATT_TH) void k_attention_seg(const AttnArgs a, const AttnBlock* __restrict__ blocks, uint32_t Tp) {
    LH_TOUCH_ARGS(a.q, a.rows, blocks);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ uint32_t Tsh[QB];
    __shared__ float invs[QB];
    constexpr int NWV = ATT_TH / 64, NG = ATT_TH / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t h = blockIdx.x;
    const AttnBlock blk = blocks[blockIdx.y];
    const uint32_t row0 = blk.row0, nb = blk.n < (uint32_t)QB ? blk.n : (uint32_t)QB;
    uint32_t T[QB], Tmax = 0;   // keys visible to row i of the block (0: no such row)
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        T[i] = (uint32_t)i < nb ? a.rows[row0 + i].pos + 1 : 0u;
        Tmax = T[i] > Tmax ? T[i] : Tmax;
    }
    if (tid < QB) Tsh[tid] = (uint32_t)tid < nb ? a.rows[row0 + tid].pos + 1 : 0u;
    float* sc = (float*)smem_raw;               // [QB][Tp] scaled scores
    float* pr = sc + (size_t)QB * Tp;           // [QB][Tp] un-normalised probabilities
    float* scratch = pr + (size_t)QB * Tp;      // [QB][ATT_TH] PV partials / reduction scratch
    const uint32_t d = a.d, hd = a.hd;
    const float* q0 = a.q + (size_t)row0 * d + h * hd;
    typedef const float __attribute__((address_space(1))) gfl;   // (global, not flat: see k_attention)
    typedef const f4 __attribute__((address_space(1))) gf4;
    gfl* Kc = (gfl*)(uintptr_t)(a.rows[row0].kc + a.kv_off + h * hd);
    gfl* Vc = (gfl*)(uintptr_t)(a.rows[row0].vc + a.kv_off + h * hd);
    const uint32_t phases = ATT_TH / hd;
    const uint32_t c = tid % hd, ph = tid / hd;
    constexpr int VP = 8;
    float vpre[VP];
#pragma unroll
    for (int k = 0; k < VP; ++k) {   // first V rows: issued before anything else, consumed last
        const uint32_t t = ph + (uint32_t)k * phases;
        vpre[k] = t < Tmax ? Vc[(size_t)t * d + c] : 0.f;
    }
    // --- scores: one key per 32-lane group, UN keys in flight per group, every K row used for all the block's queries
    const int g = tid >> 5, gl = tid & 31;
    constexpr int UN = 4;
    if (hd == 128) {
        f4 qv[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) qv[i] = (uint32_t)i < nb ? *(const f4*)(q0 + (size_t)i * d + gl * 4) : f4{0.f, 0.f, 0.f, 0.f};
        for (uint32_t t0 = g; t0 < Tmax; t0 += NG * UN) {
            f4 kv[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const uint32_t t = t0 + u * NG;
                kv[u] = *(gf4*)(Kc + (size_t)(t < Tmax ? t : 0) * d + gl * 4);
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const uint32_t t = t0 + u * NG;
#pragma unroll
                for (int i = 0; i < QB; ++i) {
                    if ((uint32_t)i >= nb) continue;   // (uniform: a short block - a decode row is a block of one - pays for its own rows only)
                    float s = fmaf(kv[u].x, qv[i].x, 0.f);
                    s = fmaf(kv[u].y, qv[i].y, s); s = fmaf(kv[u].z, qv[i].z, s); s = fmaf(kv[u].w, qv[i].w, s);
                    s = half_wave_sum(s);
                    if (gl == 0 && t < T[i]) sc[(size_t)i * Tp + t] = __fmul_rn(s, a.scale);  // Scale ml.go:2331-2374
                }
            }
        }
    } else {   // other head sizes (the small test shapes): a head of up to 128 floats is one float4 per lane, loaded once; wider heads re-read the row per query
        for (uint32_t t = g; t < Tmax; t += NG) {
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                if ((uint32_t)i >= nb) continue;
                float s = 0.f;
                for (uint32_t cc = gl * 4; cc < hd; cc += 128) {
                    const f4 kv = *(gf4*)(Kc + (size_t)t * d + cc);
                    const f4 qv = *(const f4*)(q0 + (size_t)i * d + cc);
                    s = fmaf(kv.x, qv.x, s); s = fmaf(kv.y, qv.y, s); s = fmaf(kv.z, qv.z, s); s = fmaf(kv.w, qv.w, s);
                }
                s = half_wave_sum(s);
                if (gl == 0 && t < T[i]) sc[(size_t)i * Tp + t] = __fmul_rn(s, a.scale);
            }
        }
    }
    __syncthreads();
    // --- softmax (ml.go:2432-2505) per row, the branch the per-row kernel takes for the row's T.
    // T <= 128: one wave per row.  k_attention's two short branches take the maximum and the sum with wave-level reductions over "lane, lane + 64" (every
    // wave the same code -> the same bits whichever wave runs it) and the f64 exponentials once per key.
    if (wave < QB) {
        const uint32_t Ti = Tsh[wave];
        if (Ti && Ti <= 128) {
            float* scw = sc + (size_t)wave * Tp;
            float* prw = pr + (size_t)wave * Tp;
            const uint32_t t1 = (uint32_t)lane + 64u;
            float m;
            if (Ti <= 64) m = (uint32_t)lane < Ti ? scw[lane] : -INFINITY;
            else {
                m = -INFINITY;
                for (uint32_t t = lane; t < Ti; t += 64) m = fmaxf(m, scw[t]);
            }
            m = wave_max(m);
            float psum = 0.f;
            if ((uint32_t)lane < Ti) {
                const float p = (float)exp((double)__fsub_rn(scw[lane], m));
                prw[lane] = p;
                psum += p;
            }
            if (t1 < Ti) {
                const float p = (float)exp((double)__fsub_rn(scw[t1], m));
                prw[t1] = p;
                psum += p;
            }
            psum = wave_sum(psum);
            if (lane == 0) invs[wave] = __fdiv_rn(1.0f, psum);
        }
    }
    // longer rows: the f64 exps spread over all threads, two block reductions in fixed order (k_attention's third branch), row after row
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        if (T[i] <= 128) continue;   // (uniform: the barriers below are taken by every thread or by none)
        float* sci = sc + (size_t)i * Tp;
        float* pri = pr + (size_t)i * Tp;
        float m = -INFINITY;
        for (uint32_t t = tid; t < T[i]; t += ATT_TH) m = fmaxf(m, sci[t]);
        m = wave_max(m);
        if (lane == 0) scratch[wave] = m;
        __syncthreads();
        m = scratch[0];
#pragma unroll
        for (int w = 1; w < NWV; ++w) m = fmaxf(m, scratch[w]);
        __syncthreads();
        float psum = 0.f;
        for (uint32_t t = tid; t < T[i]; t += ATT_TH) {
            const float p = (float)exp((double)__fsub_rn(sci[t], m));
            pri[t] = p;
            psum += p;
        }
        psum = wave_sum(psum);
        if (lane == 0) scratch[wave] = psum;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) tot += scratch[w];
        if (tid == 0) invs[i] = __fdiv_rn(1.0f, tot);
        __syncthreads();
    }
    __syncthreads();
    // --- PV: thread (c, ph) accumulates its key phase for every row of the block from ONE load of each V row
    float inv[QB], acc[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) { inv[i] = (uint32_t)i < nb ? invs[i] : 0.f; acc[i] = 0.f; }
#pragma unroll
    for (int k = 0; k < VP; ++k) {
        const uint32_t t = ph + (uint32_t)k * phases;
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (t < T[i]) acc[i] = fmaf(vpre[k], __fmul_rn(pr[(size_t)i * Tp + t], inv[i]), acc[i]);
    }
    for (uint32_t t0 = ph + VP * phases; t0 < Tmax; t0 += VP * phases) {
        float vv[VP];
#pragma unroll
        for (int k = 0; k < VP; ++k) {
            const uint32_t t = t0 + (uint32_t)k * phases;
            vv[k] = Vc[(size_t)(t < Tmax ? t : 0) * d + c];
        }
#pragma unroll
        for (int k = 0; k < VP; ++k) {
            const uint32_t t = t0 + (uint32_t)k * phases;
#pragma unroll
            for (int i = 0; i < QB; ++i)
                if (t < T[i]) acc[i] = fmaf(vv[k], __fmul_rn(pr[(size_t)i * Tp + t], inv[i]), acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < QB; ++i) scratch[i * ATT_TH + tid] = acc[i];
    __syncthreads();
    if (tid < (int)hd) {
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            if ((uint32_t)i >= nb) continue;
            float o = scratch[i * ATT_TH + tid];
            for (uint32_t p2 = 1; p2 < phases; ++p2) o += scratch[i * ATT_TH + tid + p2 * hd];
            const size_t idx = (size_t)(row0 + i) * d + h * hd + tid;
            a.out[idx] = o;
            if (a.out_s3) attn_store_split3(a, idx, o);
        }
    }
}

// Long contexts (plans with split partials: ctx > 256, hd = 128).  grid = (H, chunks up to the pass's highest position, blocks): a feed is not captured,
// so the grid follows the pass.  Writes the same {o[hd], m, l} partial records at the same [row][H][nch][hd + 2] addresses as k_attention_split (nch =
// the plan's chunk count); k_attention_combine then runs on the pass's row table unchanged.
template <int QB>
__global__ __launch_bounds__(ATT_TH) __attribute__((amdgpu_waves_per_eu(QB <= 4 ? 8 : 4, QB <= 4 ? 8 : 4))) void k_attention_split_seg(const AttnArgs a, const AttnBlock* __restrict__ blocks, float* __restrict__ part, uint32_t nch) {
    LH_TOUCH_ARGS(a.q, a.rows, blocks);
    __shared__ float sc[QB][ATT_TC];
    __shared__ float pr[QB][ATT_TC];
    __shared__ float scratch[QB][ATT_TH];
    __shared__ float stat[QB][2];
    __shared__ uint32_t Tsh[QB];
    constexpr int NG = ATT_TH / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t h = blockIdx.x, ch = blockIdx.y, c0 = ch * ATT_TC;
    const AttnBlock blk = blocks[blockIdx.z];
    const uint32_t row0 = blk.row0, nb = blk.n < (uint32_t)QB ? blk.n : (uint32_t)QB;
    uint32_t Tl[QB], Tlmax = 0;   // keys of this chunk visible to row i (0: the row does not reach the chunk, or no such row)
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        const uint32_t Ti = (uint32_t)i < nb ? a.rows[row0 + i].pos + 1 : 0u;
        Tl[i] = Ti <= c0 ? 0u : (Ti - c0 < (uint32_t)ATT_TC ? Ti - c0 : (uint32_t)ATT_TC);
        Tlmax = Tl[i] > Tlmax ? Tl[i] : Tlmax;
    }
    if (Tlmax == 0) return;
    if (tid < QB) {
        const uint32_t Ti = (uint32_t)tid < nb ? a.rows[row0 + tid].pos + 1 : 0u;
        Tsh[tid] = Ti <= c0 ? 0u : (Ti - c0 < (uint32_t)ATT_TC ? Ti - c0 : (uint32_t)ATT_TC);
    }
    const uint32_t d = a.d, hd = a.hd;
    const float* q0 = a.q + (size_t)row0 * d + h * hd;
    typedef const float __attribute__((address_space(1))) gfl;   // (global, not flat: see k_attention)
    typedef const f4 __attribute__((address_space(1))) gf4;
    gfl* Kc = (gfl*)(uintptr_t)(a.rows[row0].kc + a.kv_off + (size_t)c0 * d + h * hd);
    gfl* Vc = (gfl*)(uintptr_t)(a.rows[row0].vc + a.kv_off + (size_t)c0 * d + h * hd);
    const uint32_t phases = ATT_TH / hd, c = tid % hd, ph = tid / hd;
    constexpr int VP = ATT_TC / 8;  // hd = 128: 8 phases x 16 keys = the whole chunk in flight
    constexpr bool V_LATE = QB > 1 && QB <= 4;   // (see below)
    float vpre[VP];
    if (!V_LATE) {
#pragma unroll
        for (int k = 0; k < VP; ++k) {
            const uint32_t t = ph + (uint32_t)k * phases;
            vpre[k] = t < Tlmax ? Vc[(size_t)t * d + c] : 0.f;
        }
    }
    const int g = tid >> 5, gl = tid & 31;
    {   // scores of the chunk in one batch: 32 groups x 4 keys, all K rows requested before the first is used, each used for every query of the block
        constexpr int UN = ATT_TC / NG;
        f4 qv[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) qv[i] = (uint32_t)i < nb ? *(const f4*)(q0 + (size_t)i * d + gl * 4) : f4{0.f, 0.f, 0.f, 0.f};
        f4 kv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const uint32_t t = g + u * NG;
            kv[u] = *(gf4*)(Kc + (size_t)(t < Tlmax ? t : 0) * d + gl * 4);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const uint32_t t = g + u * NG;
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                if ((uint32_t)i >= nb) continue;   // (uniform: a short block pays for its own rows only)
                float s = fmaf(kv[u].x, qv[i].x, 0.f);
                s = fmaf(kv[u].y, qv[i].y, s); s = fmaf(kv[u].z, qv[i].z, s); s = fmaf(kv[u].w, qv[i].w, s);
                s = half_wave_sum(s);
                if (gl == 0 && t < Tl[i]) sc[i][t] = __fmul_rn(s, a.scale);  // Scale ml.go:2331-2374
            }
        }
    }
    __syncthreads();
    if (V_LATE) {
        // QB = 2 / 4: the V rows are requested only now, behind the barrier, so that the queries and the K rows of the score phase and the sixteen V rows
        // never hold registers together: the kernel stays within 64 VGPRs = TWO workgroups per CU (the other workgroup's work hides the V latency)
#pragma unroll
        for (int k = 0; k < VP; ++k) {
            const uint32_t t = ph + (uint32_t)k * phases;
            vpre[k] = t < Tlmax ? Vc[(size_t)t * d + c] : 0.f;
        }
    }
    // chunk-local softmax statistics of row i on wave i: maximum and sum over "lane, lane + 64" with wave-level reductions, as every wave of
    // k_attention_split computes them (same code -> same bits); the f64 exponentials once per key
    if (wave < QB) {
        const uint32_t Ti = Tsh[wave];
        if (Ti) {
            const uint32_t t1 = (uint32_t)lane + 64u;
            float m = -INFINITY;
            for (uint32_t t = lane; t < Ti; t += 64) m = fmaxf(m, sc[wave][t]);
            m = wave_max(m);
            float psum = 0.f;
            if ((uint32_t)lane < Ti) {
                const float p = (float)exp((double)__fsub_rn(sc[wave][lane], m));
                pr[wave][lane] = p;
                psum += p;
            }
            if (t1 < Ti) {
                const float p = (float)exp((double)__fsub_rn(sc[wave][t1], m));
                pr[wave][t1] = p;
                psum += p;
            }
            psum = wave_sum(psum);
            if (lane == 0) { stat[wave][0] = m; stat[wave][1] = psum; }
        }
    }
    __syncthreads();
    float acc[QB];
#pragma unroll
    for (int i = 0; i < QB; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < VP; ++k) {
        const uint32_t t = ph + (uint32_t)k * phases;
#pragma unroll
        for (int i = 0; i < QB; ++i)
            if (t < Tl[i]) acc[i] = fmaf(vpre[k], pr[i][t], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < QB; ++i) scratch[i][tid] = acc[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        if (Tl[i] == 0) continue;
        float* dst = part + (((size_t)(row0 + i) * gridDim.x + h) * nch + ch) * (hd + 2);
        if (tid < (int)hd) {
            float o = scratch[i][tid];
            for (uint32_t p2 = 1; p2 < phases; ++p2) o += scratch[i][tid + p2 * hd];
            dst[tid] = o;
        }
        if (tid == 0) { dst[hd] = stat[i][0]; dst[hd + 1] = stat[i][1]; }
    }
}

}  // namespace lh
