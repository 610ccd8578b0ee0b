// csrc/kernels_attn_share.h — tick attention of pods that share a prompt prefix (lh_batch_fork): k_attention_split on the tick's static grid, with the
// full key chunks INSIDE a sharing group's prefix read once per block of up to QB member rows instead of once per row.
// Every member of a group holds byte-equal K / V rows [0, len) in its own cache (the fork copied them; the batch drops a pod from its group when
// anything writes below len), so the partial {o[hd], m, l} of row r for such a chunk can be computed from ANY member's copy: the block's first row
// loads the chunk from ITS OWN cache and writes the partial of every row of the block into that row's slot part[(row * H + h) * nch + ch], the other
// rows of the block return at once for these chunks.  Chunks beyond the prefix, rows without a block: one row per workgroup, as k_attention_split.
// k_attention_combine then runs unchanged.
// The HARD REQUIREMENT of kernels_attn_seg.h applies word for word: per query row the operations and their order are those of k_attention_split -
// the scores through half_wave_sum, the chunk-local maximum and sum with the same lane -> key mapping, the f64 exponentials, the key-phase order
// of the PV sums, the cross-phase sum - so every partial is BIT-identical to the per-row kernel's (tests/test_gpu_batch_fork.py compares ticks byte
// for byte; LLAMAHIP_SHARE_ROW_ATTN=1 is the switch).  The body is k_attention_split_seg's with the block's rows a LIST (members of a group need not
// be neighbours in the row table) and a row's keys masked at its own position (Tl): a row that does not cover a chunk is skipped, never trusted.
#pragma once
#include "kernels_attn_seg.h"
#include "share_schedule.h"

namespace lh {

// the device table of a batch: row -> its block (SHARE_NO_BLOCK: none), and the blocks (share_schedule.h).  Written by k_share_set only.
struct ShareTable {
    uint32_t row_block[SHARE_ROWS_MAX];
    lh_share_block blocks[SHARE_BLOCKS_MAX];
};
static_assert(SHARE_CHUNK == (uint32_t)ATT_TC, "share_schedule.h counts the chunks of k_attention_split");
static_assert(sizeof(ShareTable) % 4 == 0 && sizeof(ShareTable) <= 2048, "the table travels as kernel arguments");

// One word per thread; the table travels as kernel arguments (like k_batch_set's), so a re-send needs no staging buffer and no stream wait.
__global__ __launch_bounds__(512) void k_share_set(ShareTable* __restrict__ dst, const ShareTable v) {
    const uint32_t i = threadIdx.x;
    if (i < sizeof(ShareTable) / 4) ((uint32_t*)dst)[i] = ((const uint32_t*)&v)[i];
}

// grid = (H, ceil(ctx / ATT_TC), rows), 1024 threads: the tick's static grid, so one captured graph serves every position and every table.
template <int QB>
__global__ __launch_bounds__(ATT_TH) __attribute__((amdgpu_waves_per_eu(QB <= 4 ? 8 : 4, QB <= 4 ? 8 : 4))) void k_attention_split_shared(const AttnArgs a, const ShareTable* __restrict__ tab, float* __restrict__ part) {
    LH_TOUCH_ARGS(a.q, a.rows, tab);
    static_assert(QB <= (int)SHARE_QB_MAX, "rows of a block");
    __shared__ float sc[QB][ATT_TC];
    __shared__ float pr[QB][ATT_TC];
    __shared__ float scratch[QB][ATT_TH];
    __shared__ float stat[QB][2];
    __shared__ uint32_t Tsh[QB];
    constexpr int NG = ATT_TH / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t h = blockIdx.x, ch = blockIdx.y, nch = gridDim.y, j = blockIdx.z, nrows = gridDim.z, c0 = ch * ATT_TC;
    // who computes what (uniform: everything below comes from kernel arguments and the block index)
    uint32_t rowi[QB], nb = 1;
#pragma unroll
    for (int i = 0; i < QB; ++i) rowi[i] = j;
    const uint32_t bi = tab->row_block[j];
    if (bi < SHARE_BLOCKS_MAX && ch < tab->blocks[bi].chunks) {
        const lh_share_block* blk = &tab->blocks[bi];
        if (blk->row[0] != j) return;   // the block's first row computes this chunk for me
        nb = blk->n < (uint32_t)QB ? blk->n : (uint32_t)QB;
#pragma unroll
        for (int i = 1; i < QB; ++i) rowi[i] = (uint32_t)i < nb ? blk->row[i] : j;
    }
    uint32_t Tl[QB], Tlmax = 0;   // keys of this chunk visible to row i of the block (0: the row does not reach the chunk, or no such row)
#pragma unroll
    for (int i = 0; i < QB; ++i) {
        const uint32_t Ti = ((uint32_t)i < nb && rowi[i] < nrows) ? a.rows[rowi[i]].pos + 1 : 0u;
        Tl[i] = Ti <= c0 ? 0u : (Ti - c0 < (uint32_t)ATT_TC ? Ti - c0 : (uint32_t)ATT_TC);
        Tlmax = Tl[i] > Tlmax ? Tl[i] : Tlmax;
    }
    if (Tlmax == 0) return;
    if (tid < QB) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < QB; ++i) if (tid == i) t = Tl[i];
        Tsh[tid] = t;
    }
    const uint32_t d = a.d, hd = a.hd;
    typedef const float __attribute__((address_space(1))) gfl;   // (global, not flat: see k_attention)
    typedef const f4 __attribute__((address_space(1))) gf4;
    gfl* Kc = (gfl*)(uintptr_t)(a.rows[j].kc + a.kv_off + (size_t)c0 * d + h * hd);   // my OWN cache: no pod depends on another's cache staying alive
    gfl* Vc = (gfl*)(uintptr_t)(a.rows[j].vc + a.kv_off + (size_t)c0 * d + h * hd);
    const uint32_t phases = ATT_TH / hd, c = tid % hd, ph = tid / hd;
    constexpr int VP = ATT_TC / 8;  // hd = 128: 8 phases x 16 keys = the whole chunk in flight
    constexpr bool V_LATE = QB <= 4;   // (see k_attention_split_seg: the V rows behind the barrier keep QB <= 4 within 64 VGPRs = TWO workgroups per CU)
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
        for (int i = 0; i < QB; ++i) qv[i] = Tl[i] ? *(const f4*)(a.q + (size_t)rowi[i] * d + h * hd + gl * 4) : f4{0.f, 0.f, 0.f, 0.f};
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
                if (Tl[i] == 0) continue;   // (uniform: a row on its own - every chunk beyond the prefix - pays for itself only)
                float s = fmaf(kv[u].x, qv[i].x, 0.f);
                s = fmaf(kv[u].y, qv[i].y, s); s = fmaf(kv[u].z, qv[i].z, s); s = fmaf(kv[u].w, qv[i].w, s);
                s = half_wave_sum(s);
                if (gl == 0 && t < Tl[i]) sc[i][t] = __fmul_rn(s, a.scale);  // Scale ml.go:2331-2374
            }
        }
    }
    __syncthreads();
    if (V_LATE) {
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
        if (Tl[i] == 0) continue;   // (Tl > 0 implies rowi[i] < nrows: the slot lies inside part[rows][H][nch][hd + 2])
        float* dst = part + (((size_t)rowi[i] * gridDim.x + h) * nch + ch) * (hd + 2);
        if (tid < (int)hd) {
            float o = scratch[i][tid];
            for (uint32_t p2 = 1; p2 < phases; ++p2) o += scratch[i][tid + p2 * hd];
            dst[tid] = o;
        }
        if (tid == 0) { dst[hd] = stat[i][0]; dst[hd + 1] = stat[i][1]; }
    }
}

}  // namespace lh
