// csrc/kernels_gemm_f16.h — k_gemm_b9_h: k_gemm_b9 (kernels_gemm_b9.h) over a weight matrix kept f16 in HBM (dtype 1; DESIGN 3k "Native tile GEMM").
//     Y_g[n][m] (+ R_g[n][m]) = sum_k X[n][k] * float(W_g[m][k])
// The fp32 kernel over the widened matrix issues eight bf16 products per (x tile, w tile), in the order
//     (xl,wm) (xm,wl) (xl,wh) (xm,wm) (xh,wl) (xm,wh) (xh,wm) (xh,wh).
// A widened half has at most 11 significant bits, so split3 gives it hi (8 bits), mid (at most 3 bits) and lo = +0 - for every finite half, checked over
// all 65 536 patterns on the CPU (gemm_f16_layout.h, tests/test_f16_tiles_cpu.py).  The two MFMAs that read the wl plane add exact zeros: +-0 products,
// summed to a zero, added to an accumulator that started at +0 and therefore never holds -0 - every accumulator keeps its value.  Leaving them out leaves
// each accumulator's sequence of non-zero additions as it was: the fp32 kernel's result bit for bit with SIX MFMAs (NPR = 6; NPR = 8 issues the two with
// a zero operand in their places - the fallback of DESIGN's decision rule).
//
// Everything that decides which products meet in which accumulator in which order is k_gemm_b9's: the shape of its product instantiation <1, 8, 4, 1, .>
// (128 x 256 tiles, eight waves of 128 x 32), persistent workgroups, the XCD-aware tile order, the split-K deal (sl0, nk), the 32-column slab, its two
// k-steps, the lane map of both operands, GemmArgs, gemm_store / gemm_store_fused and, through the launcher, k_split3_rows in front and k_splitk_reduce
// behind.  kernels_gemm_b9.h stays as it is; restated here: the loop, because the weight side of it differs -
//   * the W slab holds halves, [256 rows][32 halves], 64-byte rows: an X plane's geometry, swizzle and ds_read_b128 pattern (gemm_f16_layout.h).  A lane's
//     8 halves of a k-step are ONE LDS read (fp32: two);
//   * a 1 KB DMA instruction covers 16 weight rows: 24 X pieces + 16 W pieces = 40 = 5 per wave, no surplus slot (fp32: 56 = 7 per wave).  The counted
//     vmcnt waits are PPW x stages, as there;
//   * a stage is 40 KB (fp32: 56): three fit.  The ring depth NST is not part of the sums;
//   * a weight fragment is widen (v_cvt_f32_f16, f16 denormals kept, as k_gemv_sa_h), r1 = w - (w & 0xffff0000), and the high halves of w and r1 packed
//     with k_gemm_b9's byte-permute: 8 x 3 + 4 x 2 = 32 vector instructions per fragment (fp32: 44), no third part, no lo register;
//   * 24 MFMAs per k-step (NPR = 6) with the preparation work rebalanced behind them (NMF, BQ, NPC, vs below).
//
// Addresses.  X planes: k_gemm_b9's (row n >= N -> N - 1, slab past the range -> its last slab).  W: tile row m >= M -> M - 1 (virtual row 2 F - 1 for
// GEMM_EPI_SILU_MUL), so the row offset is at most (M - 1) * ldw halves; slab index sl0 + min(slab, nk - 1) <= K / 32 - 1 and source granule <= 3, so the
// column offset is at most (K / 32 - 1) * 64 + 48 bytes and the 16 bytes fetched end at (K / 32) * 64 = 2 K bytes of the row: every DMA reads inside
// [M][K] x 2 bytes (ldw = K; the launcher admits no other pitch).  LDS: piece p, lane i writes [1024 p + 16 i, + 16) with p < 40 - inside the stage.
// Values: the contract of kernels_gemm_b9.h, unchanged.  Every finite half, subnormals included, widens to 0 or a magnitude >= 2^-24 and its parts are >=
// 2^-24 too: inside split_exact_values' range.  An infinite or NaN half is outside it, as an infinite fp32 weight is (its parts are NaN).
#pragma once
#include "kernels_gemm_b9.h"
#include "gemm_f16_layout.h"

namespace lh {

__host__ __device__ constexpr size_t gemm_b9_h_lds_bytes(int nst) { return (size_t)nst * GH_STAGE; }

template <int WN, int WM, int TN, int TM, int NST, int NPR = 6>
__global__ __launch_bounds__(WN * WM * 64) void k_gemm_b9_h(const GemmArgs a) {
    static_assert(WN == 1 && WM == 8 && TN == 4 && TM == 1, "the product shape of k_gemm_b9");
    static_assert(NPR == 6 || NPR == 8, "products");
    static_assert(NST >= 2, "ring");
    constexpr int NWV = WN * WM;
    constexpr int BN = GH_BN, BM = GH_BM;
    constexpr int XP_BYTES = GH_XP_BYTES, STAGE = GH_STAGE;
    constexpr int XPIECES = GH_XPIECES, PIECES = GH_PIECES, PPW = PIECES / NWV;
    static_assert(PPW * NWV == PIECES, "no surplus slot");
    extern __shared__ __attribute__((aligned(16))) char smem_b9h[];  // [NST][STAGE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave / WM, wm = wave % WM;
    const uint32_t tiles_n = (a.N + BN - 1) / BN, tiles_m = (a.M + BM - 1) / BM;
    const uint32_t splits = a.splits ? a.splits : 1;
    const uint32_t per_group = tiles_n * tiles_m, total = per_group * a.groups * splits;
    const uint32_t ldw = a.ldw ? a.ldw : a.K;
    const int li = lane & 31, lh = lane >> 5;
    const uint32_t nkf = a.K / GBK;
    const uint32_t G = gridDim.x;
    const uint32_t v0 = (G % 8 == 0) ? (blockIdx.x % 8) * (G / 8) + blockIdx.x / 8 : blockIdx.x;
    for (uint32_t wv = v0; wv < total; wv += G) {
        const uint32_t ks = wv % splits, wi = wv / splits;
        const uint32_t g = wi / per_group, t = wi % per_group;
        const uint32_t tm = t / tiles_n, tn = t % tiles_n;
        const uint32_t n0 = tn * BN, m0 = tm * BM;
        const uint32_t sl0 = (uint32_t)(((uint64_t)ks * nkf) / splits), nk = (uint32_t)(((uint64_t)(ks + 1) * nkf) / splits) - sl0;   // first slab, slabs
        __builtin_amdgcn_s_barrier();  // every wave is done reading the previous tile's stages
        // piece p of a slab is fetched by wave p % NWV: this lane's source pointer and LDS offset for each of its pieces.  Both operands advance 64 bytes
        // per slab (32 bf16 | 32 halves).
        const char* src[PPW];
        uint32_t dst[PPW];
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp) {
            const uint32_t p = (uint32_t)wave + (uint32_t)NWV * pp;
            const uint32_t row = gemm_h_piece_row(p, (uint32_t)lane), gs = gemm_h_piece_granule(p, (uint32_t)lane);
            if (p < (uint32_t)XPIECES) {
                const uint32_t pl = p / (BN / 16), n = n0 + row;
                src[pp] = (const char*)(a.xs + (size_t)pl * a.xs_plane + (size_t)(n < a.N ? n : a.N - 1) * a.ldxs) + gs * 16;
            } else {
                const uint32_t m = m0 + row, mm = m < a.M ? m : a.M - 1;
                if (a.epi == GEMM_EPI_SILU_MUL)   // virtual row mm = row mm >> 1 of w1 (even) / w3 (odd); base + distance, never a pointer select
                    src[pp] = (const char*)((const uint16_t*)((uint64_t)a.w[0] + ((mm & 1u) ? (uint64_t)a.w[1] - (uint64_t)a.w[0] : 0)) + (size_t)(mm >> 1) * ldw) + gs * 16;
                else
                    src[pp] = (const char*)((const uint16_t*)a.w[g] + (size_t)mm * ldw) + gs * 16;
            }
            dst[pp] = gemm_h_piece_dst(p, 0);
        }
        // (the DMA is inline asm on purpose, see kernels_gemm_b9.h: through the builtin the compiler drains every DMA in flight in front of the next operand read)
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem_b9h;
        uint32_t dstS[PPW];                                                   // wave-uniform: kept in scalar registers
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp) dstS[pp] = (uint32_t)__builtin_amdgcn_readfirstlane((int)dst[pp]);
        auto issue1 = [&](uint32_t slab, int pp) {
            const uint32_t ksl = sl0 + (slab < nk ? slab : nk - 1);           // past the end: the last slab again (keeps the counts uniform; harmless)
            const uint32_t st = lds0 + (slab % NST) * STAGE;
            const char* sp = src[pp] + (size_t)ksl * (GBK * 2);
            const uint32_t m0v = st + dstS[pp];
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(m0v), "v"(sp) : "memory", "m0");
        };
        auto issue = [&](uint32_t slab) {
#pragma unroll
            for (int pp = 0; pp < PPW; ++pp) issue1(slab, pp);
        };
        f16v acc[TN][TM];
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        const uint32_t xrow = (uint32_t)(wn * TN * 32 + li) * 64, xsw = ((uint32_t)li >> 2) & 3u;
        // k_gemm_b9's software pipeline over the k-steps, scheduled by hand: while step s multiplies out of registers the operands of step s + 1 are read
        // and its weight fragment split, a few instructions behind each MFMA, every group fenced by sched_barrier(0); the slab switch inside the second
        // step of a slab after its first BQ MFMAs.
        u4 xa[2][3][TN], wq[2][2][TM];     // [operand set][plane][tile]: two weight planes
        u4 wr[TM];                         // the 8 halves of the step being prepared
        uint32_t sb[2][TM][8];             // their widened value / remainder before packing
        auto read_w = [&](uint32_t slab, int kk, int j) {
            const char* st = smem_b9h + (size_t)(slab % NST) * STAGE;
            wr[j] = *(const u4*)(st + gemm_h_w_read_off((uint32_t)(wm * TM + j), (uint32_t)li, (uint32_t)lh, (uint32_t)kk));
        };
        auto read_x = [&](int set, uint32_t slab, int kk, int pl, int i) {
            const char* st = smem_b9h + (size_t)(slab % NST) * STAGE;
            xa[set][pl][i] = *(const u4*)(st + pl * XP_BYTES + xrow + i * 32 * 64 + (((uint32_t)(2 * kk + lh)) ^ xsw) * 16);
        };
        auto split_f = [&](int j, int f) {              // 3 vector instructions: widen, and, subtract
            const uint32_t d = f / 2 == 0 ? wr[j].x : f / 2 == 1 ? wr[j].y : f / 2 == 2 ? wr[j].z : wr[j].w;
            gemm_h_split((uint16_t)((f & 1) ? d >> 16 : d & 0xffffu), &sb[0][j][f], &sb[1][j][f]);
        };
        auto pack2 = [&](int set, int j, int c) {       // 2 byte-permutes: dwords 2 (c & 1), 2 (c & 1) + 1 of plane c / 2 (4 calls per fragment)
            const int pl = c >> 1, d = (c & 1) * 2;
            uint32_t* o = (uint32_t*)&wq[set][pl][j];
            o[d] = __builtin_amdgcn_perm(sb[pl][j][2 * d + 1], sb[pl][j][2 * d], 0x07060302u);
            o[d + 1] = __builtin_amdgcn_perm(sb[pl][j][2 * d + 3], sb[pl][j][2 * d + 2], 0x07060302u);
        };
        constexpr int NMF = NPR * TN * TM, NDS = 3 * TN + TM, NPC = 12 * TM;   // MFMAs, LDS reads, vector pieces (8 splits + 4 packs per fragment)
        constexpr int BQ = NMF / 4;
        // k_gemm_b9's product order (its rows 1..8 of PX / PW) without the two products of the wl plane - or with a zero operand in their places
        auto mfma_q = [&](int set, int q) {
            constexpr int PX8[8] = {2, 1, 2, 1, 0, 1, 0, 0}, PW8[8] = {1, 2, 0, 1, 2, 0, 1, 0};
            constexpr int PX6[6] = {2, 2, 1, 1, 0, 0}, PW6[6] = {1, 0, 1, 0, 1, 0};
            const int r = q / (TN * TM), i = (q % (TN * TM)) / TM, j = q % TM;
            const int px = NPR == 6 ? PX6[r % 6] : PX8[r % 8], pw = NPR == 6 ? PW6[r % 6] : PW8[r % 8];
            const u4 z = {0u, 0u, 0u, 0u};
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8g, xa[set][px][i]), __builtin_bit_cast(bf16x8g, pw == 2 ? z : wq[set][pw & 1][j]), acc[i][j], 0, 0, 0);
        };
        auto piece = [&](int ns, int p) {
            if (p < 8 * TM) split_f(p / 8, p % 8);
            else pack2(ns, (p - 8 * TM) / 4, (p - 8 * TM) % 4);
        };
        // one k-step: multiply operand set `set`, prepare set ^ 1 from (slab, kk); boundary = the slab switch happens inside
        auto step = [&](int set, uint32_t slab, int kk, bool boundary, uint32_t refill) {
            const int ns = set ^ 1;
            const int q0 = boundary ? BQ : 0;                       // first MFMA that has preparation work behind it
            const int vs = TM + 2;                                  // vector work starts this many slots after the weight read
            const int nslots = NMF - q0 - vs;
            static_assert(NMF - BQ >= NDS && NMF - BQ - (TM + 2) >= 1 && NMF - BQ - 1 >= PPW, "the boundary step holds every read and every DMA");
#pragma unroll
            for (int q = 0; q < NMF; ++q) {
                if (boundary && q == q0) {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NST - 2)) : "memory");
                    barrier_lds_only();         // (+ lgkmcnt(0): this wave's own reads of slab kt are complete before anybody's DMA may overwrite it)
                    __builtin_amdgcn_sched_barrier(0);
                }
                mfma_q(set, q);
                const int e = q - q0;
                if (e >= 0) {
                    if (e < TM) read_w(slab, kk, e);
                    else if (e < NDS) read_x(ns, slab, kk, (e - TM) / TN, (e - TM) % TN);
                    if (boundary && e >= 1 && e - 1 < PPW) issue1(refill, e - 1);
                    if (e >= vs) {
                        const int s = e - vs;
#pragma unroll
                        for (int p = s * NPC / nslots; p < (s + 1) * NPC / nslots; ++p) piece(ns, p);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
#pragma unroll
        for (int j = 0; j < NST; ++j) issue((uint32_t)j);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NST - 1)) : "memory");      // slab 0 of mine
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < TM; ++j) read_w(0, 0, j);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int i = 0; i < TN; ++i) read_x(0, 0, 0, pl, i);
#pragma unroll
        for (int p = 0; p < NPC; ++p) piece(0, p);
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t kt = 0; kt < nk; ++kt) {
            step(0, kt, 1, false, 0);                                       // first step of slab kt; prepares its second step
            step(1, kt + 1 < nk ? kt + 1 : kt, 0, true, kt + NST);      // second step; prepares the first step of slab kt + 1
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail DMA
        float* Y = splits > 1 ? a.part + ((size_t)(g * splits + ks) * a.N) * a.M : a.y[g];
        const float* R = splits > 1 ? nullptr : a.r[g];
        if (splits > 1) gemm_store<TN, TM>(a, acc, Y, R, n0 + wn * TN * 32, m0 + wm * TM * 32, li, lh, a.M);
        else if (a.epi != GEMM_EPI_STORE) gemm_store_fused<TN, TM>(a, acc, g, n0 + wn * TN * 32, m0 + wm * TM * 32, li, lh);
        else gemm_store<TN, TM>(a, acc, Y, R, n0 + wn * TN * 32, m0 + wm * TM * 32, li, lh, a.ldy);
    }
}

}  // namespace lh
