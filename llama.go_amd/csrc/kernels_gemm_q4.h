// csrc/kernels_gemm_q4.h — block-int4 weights, long prompts: k_gemm_q4b3 = k_gemm_q8b3 (kernels_gemm_b9.h) reading the NIBBLE plane of a dtype-2 buffer.
//     Y[n][m] (+ R[n][m]) = sum over quant blocks b of d[m][b] * sum_{k in b} (nib[m][k] - 8) * X[n][k]
// Why: from 89 prompt rows on, a block-int4 model expanded every matrix into an int8 image (k_expand_q4: 0.5 B read + 1 B written per weight) that
// k_gemm_q8b3 then read (1 B) - 2.5 B per weight where the int8 twin moves 1 and the nibbles alone are 0.5.  A 4-bit quant n - 8 is an exact bf16 like any
// int8 quant and the scale plane of a dtype-2 buffer has the int8 buffer's shape, so this kernel differs from k_gemm_q8b3 ONLY in where a lane's sixteen
// quants of a slab come from, and feeds identical operands into the identical MFMA and fma sequence: every sum is the int8 twin's bit for bit.
//
// The same (these decide the bits; not restated, see kernels_gemm_b9.h): 128 x 256 tiles, eight waves of 128 x 32; one slab = 32 columns = one quant block;
// the X stage [3][128][32 bf16] with its swizzle and DMA pieces; the scale ring (three buffers [256][4], one granule = one row's scales of four slabs); per
// slab and wave 24 MFMAs in twelve fenced groups, low plane first, into a zeroed partial sum; one fma(ps, d, acc) per element and block; the work-item
// order; split-K ranges in whole scale groups; gemm_store<4, 1>; k_split3_rows in front and k_splitk_reduce behind.
//
// The kernel's own:
//   * W in LDS.  A slab's weights are [256 rows][16 B] = 4 KB (int8: 8 KB), kept OUTSIDE the X stages in a ring of two slab PAIRS (gemm_q4_layout.h):
//     NST x 24 KB of X + 16 KB of W + 12 KB of scales = 124 KB at NST = 4 (int8: 140 KB), 148 KB at NST = 5.
//   * DMA of W: each wave brings its OWN 32 rows, for TWO slabs in one global_load_lds_dwordx4 (lane i: row i & 31, bytes 16 (i >> 5) .. + 15 of the row's
//     32 contiguous bytes) - four wave-wide instructions per slab of the tile instead of eight, every one a full 1 KB request of 32-byte runs.  Chosen over
//     one EXEC-masked half-wave instruction per wave and slab (uniform counts, but 16 B per row and request, and twice the instructions).  The pair rides
//     with the X pieces of its EVEN slab, so a wave has 4 (+ 1: wave 0's scales) loads in flight for an even slab and 3 for an odd one, and the counted
//     s_waitcnt vmcnt(n) are compile-time constants per slab parity (q4b3_pending; slab_body is unrolled by parity as in the int8 kernel).
//     Two pair slots suffice: a wave reads only rows it fetched itself; W of slab j is read in group 8 of slab j - 1; the pair (j, j + 1), j even, is
//     issued in group 11 of slab j - NST + 1 into the slot of pair (j - 4, j - 3), whose last read - W of slab j - 3 - stood in group 8 of slab j - 4:
//     behind us for NST <= 5.  The other slot holds pair (j - 2, j - 1), which is live.  Past the end: the last pair again (uniform counts; harmless).
//   * Operand read: one ds_read_b64 per lane and slab - bytes 8 lh .. 8 lh + 7 of row li's granule = columns 16 lh .. 16 lh + 15; dword st of it holds the
//     eight nibbles of k-step st (columns 16 lh + 8 st + e, e = 0..7 in nibble order) and goes through stream_q4_operand (stream_q4_layout.h: the nibble
//     masked into an fp32 mantissa, one exact subtraction), which yields element for element what k_gemm_q8b3's convert yields for the expanded quants.
// Packed fp32 instructions are switched off for this kernel (the attribute below): fold's fma and the conversion's subtraction are then one scalar
// instruction per element - the same IEEE operations on the same values, so the bits do not depend on it.
#pragma once
#include "kernels_gemm_b9.h"
#include "gemm_q4_layout.h"
#include "stream_q4_layout.h"
#include <type_traits>

namespace lh {

typedef unsigned int u2 __attribute__((ext_vector_type(2)));   // (kernels_q4.h's)

#ifndef Q4B3_NST
#define Q4B3_NST 4   // ring depth of the X stages (no part of the sums); -DQ4B3_NST=5 through make EXTRA= is the probe build (profiles/q4_tiles.txt)
#endif
constexpr int Q4T_XSTAGE = 3 * Q3_XP;
__host__ __device__ constexpr size_t gemm_q4b3_lds_bytes(int nst) { return (size_t)nst * Q4T_XSTAGE + GEMM_Q4_W_BYTES + 3 * Q3_BM * 16; }
// DMA instructions of this wave that may still be in flight while the wave waits, in a slab of parity par, for the pieces of the slab after it: those of
// the slabs `from` .. nst - 2 ahead (3 X pieces each, + the W pair on an even slab, + wave 0's scale quarter)
__host__ __device__ constexpr int q4b3_pending(int nst, int par, bool wave0, int from) {
    int n = 0;
    for (int o = from; o <= nst - 2; ++o) n += 3 + ((o & 1) == par ? 1 : 0) + (wave0 ? 1 : 0);
    return n;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
template <int NST>
__global__ __launch_bounds__(512) void k_gemm_q4b3(const GemmArgs a) {
    static_assert(NST == 4 || NST == 5, "ring depth (two W pair slots: see above)");
    constexpr int BN = Q3_BN, BM = Q3_BM, XP_BYTES = Q3_XP, STAGE = Q4T_XSTAGE, W_OFF = NST * STAGE, S_OFF = W_OFF + (int)GEMM_Q4_W_BYTES;
    static_assert(BM == (int)GEMM_Q4_BM, "tile rows");
    extern __shared__ __attribute__((aligned(16))) char smem_q4t[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const uint32_t tiles_n = (a.N + BN - 1) / BN, tiles_m = (a.M + BM - 1) / BM;
    const uint32_t splits = a.splits ? a.splits : 1;
    const uint32_t per_group = tiles_n * tiles_m, total = per_group * a.groups * splits;
    const uint32_t nkf = a.K / GBK, ngr = nkf / 4;          // slabs and scale groups of the matrix
    const uint32_t G = gridDim.x;
    const uint32_t v0 = (G % 8 == 0) ? (blockIdx.x % 8) * (G / 8) + blockIdx.x / 8 : blockIdx.x;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem_q4t;
    for (uint32_t wv = v0; wv < total; wv += G) {
        const uint32_t ks = wv % splits, wi = wv / splits;
        const uint32_t g = wi / per_group, t = wi % per_group;
        const uint32_t tm = t / tiles_n, tn = t % tiles_n;
        const uint32_t gr0 = (uint32_t)(((uint64_t)ks * ngr) / splits), nsg = (uint32_t)(((uint64_t)(ks + 1) * ngr) / splits) - gr0;
        const uint32_t n0 = tn * BN, m0 = tm * BM, ks0 = 4 * gr0, nk = 4 * nsg;
        __builtin_amdgcn_s_barrier();  // every wave is done reading the previous tile's stages
        // this wave's DMA pieces: X row block `wave` of the three planes per slab, W rows 32 wave .. + 31 per slab PAIR, (wave 0) a slab's quarter of the scales
        const char* xsrc[3]; const char* wsrc;
        {
            const uint32_t row = (uint32_t)wave * 16 + (uint32_t)(lane >> 2), gs = (uint32_t)(lane & 3) ^ ((row >> 2) & 3u);
            const uint32_t n = n0 + row, nc = n < a.N ? n : a.N - 1;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) xsrc[pl] = (const char*)(a.xs + (size_t)pl * a.xs_plane + (size_t)nc * a.ldxs) + gs * 16 + (size_t)ks0 * 64;
            const uint32_t m = m0 + gemm_q4_dma_row((uint32_t)wave, (uint32_t)lane), mc = m < a.M ? m : a.M - 1;
            wsrc = (const char*)a.w[g] + (size_t)mc * (a.K / 2) + gemm_q4_dma_granule((uint32_t)lane) * 16 + (size_t)ks0 * 16;
        }
        auto ssrc = [&](uint32_t qd) {     // (wave 0) this lane's row of scale quarter qd
            const uint32_t sm = m0 + qd * 64 + (uint32_t)lane, smc = sm < a.M ? sm : a.M - 1;
            return (const char*)(a.ws[g] + (size_t)smc * nkf + ks0);
        };
        auto dma = [&](uint32_t m0v, const char* sp) {
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(m0v), "v"(sp) : "memory", "m0");
        };
        // piece pc of slab `slab` (0..2: X planes, 3: the W pair (slab, slab + 1) - even slabs only, 4: scales - wave 0 only)
        auto issue1 = [&](uint32_t slab, int pc) {
            const uint32_t kc = slab < nk ? slab : nk - 1;                  // past the end: the last slab again (uniform counts; harmless)
            if (pc < 3) dma(lds0 + (slab % NST) * STAGE + pc * XP_BYTES + (uint32_t)wave * 1024, xsrc[pc] + (size_t)kc * 64);
            else if (pc == 3) dma(lds0 + W_OFF + gemm_q4_w_off(slab, (uint32_t)wave * 32, 0), wsrc + (size_t)(slab < nk ? slab : nk - 2) * 16);   // (nk is a multiple of 4)
            else {
                const uint32_t sgp = slab / 4 + 1, sgc = sgp < nsg ? sgp : nsg - 1, qd = slab % 4;
                dma(lds0 + S_OFF + (sgp % 3) * (BM * 16) + qd * 1024, ssrc(qd) + (size_t)sgc * 16);
            }
        };
        f16v acc[4][1], ps[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][0][e] = 0.f; ps[i][e] = 0.f; }
        const uint32_t xrow = (uint32_t)li * 64, xsw = ((uint32_t)li >> 2) & 3u;
        const uint32_t spos = S_OFF + (uint32_t)(wave * 32 + li) * 16;
        u4 xr[4][2];            // ring of X operand pairs
        u4 wq[2][2];            // [slab parity][k-step] converted weights
        u2 raw;                 // next slab's 16 nibbles
        float dsc[2] = {0.f, 0.f};     // [slab parity] block scale of this lane's weight row
        auto read_x = [&](uint32_t slab, int grp) {   // group 0..11 of a slab -> ring slot grp % 4
            const int pr = grp / 6, sp = grp % 6, st = sp / 3, pl = 2 - sp % 3;
            const char* sb = smem_q4t + (size_t)(slab % NST) * STAGE + pl * XP_BYTES + xrow + (((uint32_t)(2 * lh + st)) ^ xsw) * 16;
            xr[grp % 4][0] = *(const u4*)(sb + (2 * pr) * 32 * 64);
            xr[grp % 4][1] = *(const u4*)(sb + (2 * pr + 1) * 32 * 64);
        };
        auto read_w = [&](uint32_t slab, int par) {
            raw = *(const u2*)(smem_q4t + W_OFF + gemm_q4_read_off(slab, (uint32_t)wave, (uint32_t)li, (uint32_t)lh));
            dsc[par] = *(const float*)(smem_q4t + spos + ((slab / 4) % 3) * (BM * 16) + (slab % 4) * 4);
        };
        auto convert = [&](int par, int part) {       // part 0 / 1: k-step's eight nibbles -> bf16, pinned where it stands
            if (part > 1) return;
            uint32_t c[4];
            stream_q4_operand(part ? raw.y : raw.x, c);
            u4 o = u4{c[0], c[1], c[2], c[3]};
            asm volatile("" : "+v"(o));
            wq[par][part] = o;
        };
        auto fold = [&](int tile, int quarter, float d) {   // acc += d * ps for four of the tile's sixteen values (k_gemm_q8b3's fma, element by element)
            const f2v d2 = {d, d};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int e = 4 * quarter + 2 * h;
                const f2v p2 = {ps[tile][e], ps[tile][e + 1]}, a2 = {acc[tile][0][e], acc[tile][0][e + 1]};
                f2v r2 = __builtin_elementwise_fma(p2, d2, a2);
                asm volatile("" : "+v"(r2));          // (keeps the FMA behind these MFMAs: left alone it sinks to the end of the loop body)
                acc[tile][0][e] = r2.x; acc[tile][0][e + 1] = r2.y;
            }
        };
        // one slab: multiply out of registers, prepare the next one
        auto slab_body = [&](uint32_t kt, auto parc, bool first) {
            constexpr int par = decltype(parc)::value;
            const uint32_t nxt = kt + 1 < nk ? kt + 1 : kt;
#pragma unroll
            for (int grp = 0; grp < 12; ++grp) {
                const int pr = grp / 6, sp = grp % 6, st = sp / 3;
                if (grp == 8) {
                    if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(q4b3_pending(NST, par, true, 2)) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(q4b3_pending(NST, par, false, 2)) : "memory");
                    barrier_lds_only();
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int tile = 2 * pr + h;
                    const f16v z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    ps[tile] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8g, xr[grp % 4][h]), __builtin_bit_cast(bf16x8g, wq[par][st]), sp == 0 ? z : ps[tile], 0, 0, 0);
                }
                if (grp + 3 < 12) read_x(kt, grp + 3); else read_x(nxt, grp + 3 - 12);
                if (grp < 4 && !first) { fold(2, grp, dsc[par ^ 1]); fold(3, grp, dsc[par ^ 1]); }          // the previous slab's pair (2, 3)
                if (grp >= 6 && grp < 10) { fold(0, grp - 6, dsc[par]); fold(1, grp - 6, dsc[par]); }
                if (grp == 8) read_w(nxt, par ^ 1);
                if (grp >= 9) convert(par ^ 1, grp - 9);
                if (grp >= 8 && grp < 11) issue1(kt + NST - 1, grp - 8);
                if (grp == 11) {
                    if constexpr (((par + NST - 1) & 1) == 0) issue1(kt + NST - 1, 3);      // slab kt + NST - 1 is even: its pair
                    if (wave == 0) issue1(kt + NST - 1, 4);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // prologue: scale group 0, slabs 0 .. NST - 2
        if (wave == 0) {
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) dma(lds0 + S_OFF + qd * 1024, ssrc((uint32_t)qd));
        }
#pragma unroll
        for (int j = 0; j < NST - 1; ++j) {
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) issue1((uint32_t)j, pc);
            if ((j & 1) == 0) issue1((uint32_t)j, 3);
            if (wave == 0) issue1((uint32_t)j, 4);
        }
        if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(q4b3_pending(NST, 0, true, 1)) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(q4b3_pending(NST, 0, false, 1)) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        read_x(0, 0); read_x(0, 1); read_x(0, 2);
        read_w(0, 0);
        convert(0, 0); convert(0, 1);
        __builtin_amdgcn_sched_barrier(0);
        slab_body(0, std::integral_constant<int, 0>{}, true);
        slab_body(1, std::integral_constant<int, 1>{}, false);
        for (uint32_t kt = 2; kt < nk; kt += 2) {
            slab_body(kt, std::integral_constant<int, 0>{}, false);
            slab_body(kt + 1, std::integral_constant<int, 1>{}, false);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { fold(2, q, dsc[1]); fold(3, q, dsc[1]); }      // the last slab's pair (2, 3)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail DMA
        if (splits > 1) gemm_store<4, 1>(a, acc, a.part + ((size_t)(g * splits + ks) * a.N) * a.M, nullptr, n0, m0 + (uint32_t)wave * 32, li, lh, a.M);
        else gemm_store<4, 1>(a, acc, a.y[g], a.r[g], n0, m0 + (uint32_t)wave * 32, li, lh, a.ldy);
    }
}
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace lh
