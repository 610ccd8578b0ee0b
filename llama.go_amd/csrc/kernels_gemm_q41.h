// csrc/kernels_gemm_q41.h — k_gemm_b9_q41: k_gemm_b9 (kernels_gemm_b9.h) over a weight matrix kept Q4_1 in HBM (dtype 3; DESIGN 3m "Native tile GEMM").
//     Y_g[n][m] (+ R_g[n][m]) = sum_k X[n][k] * w'_g[m][k],   w' = fl32(fma(d, nib, m))   (kernels_q41.h: the value k_expand_q41 writes)
// Contract: byte for byte what k_gemm_b9<1, 8, 4, 1, 2> gives over the expanded matrix.  Everything that decides which product meets which accumulator in
// which order is k_gemm_b9's and is restated unchanged: the <1, 8, 4, 1, .> shape (128 x 256 tiles, eight waves of 128 x 32), persistent workgroups, the
// XCD-aware tile order, the split-K deal (sl0, nk), two k-steps per 32-column slab, the lane map of both operands, the eight products in its order - all
// eight: w' has 24 significant bits, no plane is zero -, split3 and the byte-permute packing, GemmArgs, gemm_store / gemm_store_fused and, through the
// launcher, k_split3_rows in front and k_splitk_reduce behind.  kernels_gemm_b9.h stays as it is.
//
// The weight side is the kernel's own (gemm_q41_layout.h):
//   * HBM: a.w[g] = the nibble plane [M][K / 2], a.ws[g] = the (d, m) pair plane [M][K / 32][2] fp32.
//   * a ring stage = the three X planes (24 KB) + a nibble slab [256 rows][16 B] (4 KB) = 28 KB (fp32: 56, f16: 40); behind the NST stages a ring of
//     NST / 2 + 1 pair slots of 4 KB.
//   * DMA: every wave brings 3 X pieces per slab (its 16 rows of each plane).  Waves 0..3 bring the slab's four nibble pieces (one lane = one weight row's
//     16 bytes; fp32: 32 W pieces per slab).  Waves 4..7 bring the four pair pieces of a slab PAIR (one lane = one row's (d, m) of blocks 2 P, 2 P + 1,
//     16 contiguous bytes), with the pieces of the pair's even slab - k_gemm_q4b3's slab-pair scheme.  P = (sl0 + slab) >> 1 counts absolute slabs, so a
//     range that starts at an odd slab fetches its first pair with slab 0 and uses its second half.  A wave therefore has 4 DMAs per slab in flight
//     (waves 0..3) or 3 / 4 by the slab's absolute parity (waves 4..7), and the counted s_waitcnt vmcnt(n) are compile-time constants per wave class and
//     parity (gemm_q41_pending): the slab loop is unrolled by absolute parity, an odd first slab peeled in front of it.
//   * the pair ring's slots.  Unlike k_gemm_q4b3 a pair piece covers 64 rows = TWO waves' rows, so "a wave reads only what it fetched" does not hold here;
//     the ring lives under the stage ring's barrier instead.  Pair P (even slab s) is issued behind the barrier of slab s - NST's boundary (or in the
//     prologue) and read ONCE per wave, 16 bytes into registers, behind the barrier of slab s - 1's boundary (or in the prologue); that barrier stands
//     behind every wave's "my pieces of slab s have landed".  Its slot is written next for pair P + SLOTS, behind the barrier of slab s + 2 SLOTS - NST's
//     boundary, which every wave reaches with its LDS reads complete (lgkmcnt(0)): safe iff s + 2 SLOTS - NST >= s.  In the prologue all of slabs
//     0 .. NST - 1 are issued before anything is read; they touch at most NST / 2 + 1 consecutive pairs (an odd first slab included).  Both hold for
//     SLOTS = NST / 2 + 1.
//   * operand read: ONE ds_read_b128 per lane and slab of row 32 wave + li's 16 bytes (32 rows x 16 B dense, both wave halves at the same addresses:
//     conflict-free), dword 2 kk + lh of it picked per k-step with one v_cndmask.  Chosen over two ds_read_b32 at pitch 16 (a 2-way bank conflict each,
//     and twice the LDS instructions behind the MFMAs) - the select costs one vector instruction per fragment.  The slab's (d, m) come out of the
//     registers that hold the pair (a compile-time half per parity).
//   * unpack, per fragment of 8 weights: & 0x0f0f0f0f, >> 4 &, (k_gemv_q41s' empty asm keeps them from folding into bit-field extracts), eight
//     v_cvt_f32_ubyteN, and ONE fma per weight (the library is built with contraction off, the fma is written out) - the IEEE operation k_expand_q41
//     performs, so the eight floats are the expanded matrix's.  Scalar v_fma_f32 with d and m each in a register of its own: the packed form with both
//     broadcast out of one register pair came out of the compiler with the addend's op_sel wrong (m read as d - seen as wrong sums, then in the ISA).
//     From there k_gemm_b9's split3 (32) and packing (12): 1 + 3 + 8 + 8 + 44 = 64 vector instructions per fragment against 32 MFMAs (fp32: 44 against
//     32), spread behind the MFMAs by hand as there.
//
// Addresses.  X planes: k_gemm_b9's (row n >= N -> N - 1, slab past the range -> its last slab).  W: tile row m >= M -> M - 1 (virtual row 2 F - 1 of
// GEMM_EPI_SILU_MUL: row v >> 1 of matrix v & 1, base + distance for BOTH planes), so a row starts at most (M - 1) rows into its plane.  Nibbles: slab
// sl0 + min(slab, nk - 1) <= K / 32 - 1, 16 bytes at 16 x that: they end at most at K / 2 of the row.  Pairs: pair index (sl0 + min(slab, nk - 1)) >> 1
// <= K / 64 - 1 (K % 64 == 0: the launcher admits nothing else), 16 bytes at 16 x that: they end at most at K / 32 x 8 bytes of the row, and start 16-byte
// aligned.  LDS: X piece (plane pl, wave w) writes [pl 8192 + 1024 w, + 1024), nibble piece q [24576 + 1024 q, + 1024) - inside the 28 KB stage; pair
// piece q writes [1024 q, + 1024) of a 4 KB slot with slot < NST / 2 + 1 - inside the ring (gemm_q41_lds_bytes).
// Values: the contract of kernels_gemm_b9.h, unchanged, over the w'.
#pragma once
#include "kernels_gemm_b9.h"
#include "gemm_q41_layout.h"
#include <type_traits>

namespace lh {

#ifndef B9Q41_NST
#define B9Q41_NST 3   // ring depth (no part of the sums); -DB9Q41_NST=2 | 4 | 5 through make EXTRA= are the probe builds (profiles/q41_tiles.txt)
#endif

// DMA instructions of one wave that may still be in flight once the pieces of a slab must have landed: those of the `ahead` slabs issued behind it, the
// first of which has absolute parity ph1 (3 X pieces each + a nibble piece every slab | the pair piece on even slabs)
__host__ __device__ constexpr int gemm_q41_pending(int ahead, int ph1, bool pair_wave) {
    int n = 0;
    for (int j = 0; j < ahead; ++j) n += 3 + (pair_wave ? (((ph1 + j) & 1) == 0 ? 1 : 0) : 1);
    return n;
}

template <int WN, int WM, int TN, int TM, int NST>
__global__ __launch_bounds__(WN * WM * 64) void k_gemm_b9_q41(const GemmArgs a) {
    static_assert(WN == 1 && WM == 8 && TN == 4 && TM == 1, "the product shape of k_gemm_b9");
    static_assert(NST >= 2 && NST <= 5, "ring");
    constexpr int BN = GQ41_BN, BM = GQ41_BM, XP_BYTES = GQ41_XP_BYTES, STAGE = GQ41_STAGE;
    constexpr uint32_t P_OFF = NST * GQ41_STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem_b9q[];  // [NST][STAGE] | [pair slots][4 KB]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool pair_wave = wave >= 4;
    const uint32_t tiles_n = (a.N + BN - 1) / BN, tiles_m = (a.M + BM - 1) / BM;
    const uint32_t splits = a.splits ? a.splits : 1;
    const uint32_t per_group = tiles_n * tiles_m, total = per_group * a.groups * splits;
    const int li = lane & 31, lh = lane >> 5;
    const uint32_t nkf = a.K / GBK;
    const uint32_t G = gridDim.x;
    const uint32_t v0 = (G % 8 == 0) ? (blockIdx.x % 8) * (G / 8) + blockIdx.x / 8 : blockIdx.x;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem_b9q;
    for (uint32_t wv = v0; wv < total; wv += G) {
        const uint32_t ks = wv % splits, wi = wv / splits;
        const uint32_t g = wi / per_group, t = wi % per_group;
        const uint32_t tm = t / tiles_n, tn = t % tiles_n;
        const uint32_t n0 = tn * BN, m0 = tm * BM;
        const uint32_t sl0 = (uint32_t)(((uint64_t)ks * nkf) / splits), nk = (uint32_t)(((uint64_t)(ks + 1) * nkf) / splits) - sl0;   // first slab, slabs
        const uint32_t odd = sl0 & 1u;                                  // the range begins in the second half of a pair
        __builtin_amdgcn_s_barrier();  // every wave is done reading the previous tile's stages
        // this wave's DMA pieces: X row block `wave` of the three planes per slab; waves 0..3 nibble piece `wave` per slab, waves 4..7 pair piece wave - 4 per pair
        const char* xsrc[3]; const char* wsrc;
        {
            const uint32_t row = (uint32_t)wave * 16 + (uint32_t)(lane >> 2), gs = (uint32_t)(lane & 3) ^ ((row >> 2) & 3u);
            const uint32_t n = n0 + row, nc = n < a.N ? n : a.N - 1;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) xsrc[pl] = (const char*)(a.xs + (size_t)pl * a.xs_plane + (size_t)nc * a.ldxs) + gs * 16;
            const uint32_t m = m0 + gemm_q41_piece_row((uint32_t)wave & 3u, (uint32_t)lane), mm = m < a.M ? m : a.M - 1;
            const uint64_t rowb = pair_wave ? (uint64_t)nkf * 8u : (uint64_t)(a.K / 2);     // bytes of a row of this wave's plane
            if (a.epi == GEMM_EPI_SILU_MUL) {   // virtual row mm = row mm >> 1 of w1 (even) / w3 (odd); base + distance, never a pointer select - for both planes
                const uint64_t b0 = pair_wave ? (uint64_t)a.ws[0] : (uint64_t)a.w[0], b1 = pair_wave ? (uint64_t)a.ws[1] : (uint64_t)a.w[1];
                wsrc = (const char*)(b0 + ((mm & 1u) ? b1 - b0 : 0) + (uint64_t)(mm >> 1) * rowb);
            } else {
                wsrc = (const char*)((pair_wave ? (uint64_t)a.ws[g] : (uint64_t)a.w[g]) + (uint64_t)mm * rowb);
            }
        }
        // (the DMA is inline asm on purpose, see kernels_gemm_b9.h: through the builtin the compiler drains every DMA in flight in front of the next operand read)
        auto dma = [&](uint32_t m0v, const char* sp) {
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(__builtin_amdgcn_readfirstlane((int)m0v)), "v"(sp) : "memory", "m0");   // (m0v is wave-uniform)
        };
        // piece pc of slab `slab`: 0..2 the X planes; 3 this wave's weight piece - the slab's nibbles (waves 0..3) or, if `pair`, the pair the slab lies in
        auto issue1 = [&](uint32_t slab, int pc, bool pair) {
            const uint32_t kc = sl0 + (slab < nk ? slab : nk - 1);            // past the end: the last slab (pair) again (keeps the counts uniform; harmless)
            const uint32_t st = lds0 + (slab % NST) * STAGE;
            if (pc < 3) dma(st + pc * XP_BYTES + (uint32_t)wave * 1024, xsrc[pc] + (size_t)kc * 64);
            else if (!pair_wave) dma(st + gemm_q41_nib_dst((uint32_t)wave, 0), wsrc + (size_t)kc * 16);
            else if (pair) dma(lds0 + P_OFF + gemm_q41_pair_slot(sl0 + slab, NST) * GQ41_PAIR_BYTES + gemm_q41_pair_dst((uint32_t)wave & 3u, 0), wsrc + (size_t)(kc >> 1) * 16);
        };
        f16v acc[TN][TM];
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][0][e] = 0.f;
        const uint32_t xrow = (uint32_t)li * 64, xsw = ((uint32_t)li >> 2) & 3u;
        const uint32_t wpos = gemm_q41_w_read_off((uint32_t)wave, (uint32_t)li), ppos = P_OFF + gemm_q41_pair_read_off((uint32_t)wave, (uint32_t)li);
        // k_gemm_b9's software pipeline over the k-steps, scheduled by hand: while step s multiplies out of registers the operands of step s + 1 are read
        // and its weight fragment unpacked, dequantised and split, a few instructions behind each MFMA, every group fenced by sched_barrier(0); the slab
        // switch inside the second step of a slab after its first BQ MFMAs.
        u4 xa[2][3][TN], wq[2][3];         // [operand set][plane][tile]
        u4 nq = {0u, 0u, 0u, 0u};          // the 16 nibble bytes of the slab being prepared (this lane's weight row)
        u4 pm = {0u, 0u, 0u, 0u};          // (d, m) of the two blocks of the pair being prepared
        float dq = 0.f, mq = 0.f;          // (d, m) of the slab being prepared
        uint32_t nlo = 0, nhi = 0;         // the fragment's even / odd elements, one per byte
        float wr[8];                       // the weight floats of the step being prepared
        uint32_t sb[3][8];                 // their hi / mid / lo parts before packing
        auto read_w = [&](uint32_t slab) { nq = *(const u4*)(smem_b9q + (size_t)(slab % NST) * STAGE + wpos); };
        auto read_pm = [&](uint32_t slab) { pm = *(const u4*)(smem_b9q + ppos + gemm_q41_pair_slot(sl0 + slab, NST) * GQ41_PAIR_BYTES); };
        auto read_x = [&](int set, uint32_t slab, int kk, int pl, int i) {
            const char* st = smem_b9q + (size_t)(slab % NST) * STAGE;
            xa[set][pl][i] = *(const u4*)(st + pl * XP_BYTES + xrow + i * 32 * 64 + (((uint32_t)(2 * kk + lh)) ^ xsw) * 16);
        };
        auto nibbles = [&](int kk) {                    // 4 vector instructions: the k-step's dword (gemm_q41_frag_dword), its low and high nibbles
            const uint32_t q = kk ? (lh ? nq.w : nq.z) : (lh ? nq.y : nq.x);
            nlo = q & 0x0f0f0f0fu; nhi = (q >> 4) & 0x0f0f0f0fu;
            asm("" : "+v"(nlo), "+v"(nhi));
        };
        auto set_dm = [&](bool second) {                // the block's (d, m) out of the pair, each pinned in a register of its own
            dq = __builtin_bit_cast(float, second ? pm.z : pm.x); mq = __builtin_bit_cast(float, second ? pm.w : pm.y);
            asm("" : "+v"(dq), "+v"(mq));
        };
        auto dequant = [&](int b) {                     // byte b: elements 2 b, 2 b + 1 - two byte converts and two fma(d, n, m)
            wr[2 * b] = __builtin_fmaf(dq, (float)((nlo >> (8 * b)) & 0xffu), mq);
            wr[2 * b + 1] = __builtin_fmaf(dq, (float)((nhi >> (8 * b)) & 0xffu), mq);
        };
        auto split_f = [&](int f) {                     // 4 vector instructions (k_gemm_b9's)
            const uint32_t hb = __builtin_bit_cast(uint32_t, wr[f]) & 0xffff0000u;
            const float r1 = __fsub_rn(wr[f], __builtin_bit_cast(float, hb));
            const uint32_t mb = __builtin_bit_cast(uint32_t, r1) & 0xffff0000u;
            const float r2 = __fsub_rn(r1, __builtin_bit_cast(float, mb));
            sb[0][f] = __builtin_bit_cast(uint32_t, wr[f]); sb[1][f] = __builtin_bit_cast(uint32_t, r1); sb[2][f] = __builtin_bit_cast(uint32_t, r2);
        };
        auto pack2 = [&](int set, int c) {              // 2 byte-permutes: dwords 2 (c & 1), 2 (c & 1) + 1 of plane c / 2 (6 calls per fragment)
            const int pl = c >> 1, d = (c & 1) * 2;
            uint32_t* o = (uint32_t*)&wq[set][pl];
            o[d] = __builtin_amdgcn_perm(sb[pl][2 * d + 1], sb[pl][2 * d], 0x07060302u);
            o[d + 1] = __builtin_amdgcn_perm(sb[pl][2 * d + 3], sb[pl][2 * d + 2], 0x07060302u);
        };
        constexpr int NMF = 8 * TN, NDS = 2 + 3 * TN, NPC = 1 + 4 + 8 + 6;   // MFMAs, LDS read slots, vector pieces (nibbles, 4 dequants, 8 splits, 6 packs)
        constexpr int BQ = NMF / 4;
        // k_gemm_b9's eight products per (x tile, w tile), the small ones first (its rows 1..8 of PX / PW); consecutive MFMAs go to different accumulators
        auto mfma_q = [&](int set, int q) {
            constexpr int PX[8] = {2, 1, 2, 1, 0, 1, 0, 0}, PW[8] = {1, 2, 0, 1, 2, 0, 1, 0};
            const int r = q / TN, i = q % TN;
            acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8g, xa[set][PX[r]][i]), __builtin_bit_cast(bf16x8g, wq[set][PW[r]]), acc[i][0], 0, 0, 0);
        };
        auto piece = [&](int ns, int kk, int p) {
            if (p == 0) nibbles(kk);
            else if (p < 5) dequant(p - 1);
            else if (p < 13) split_f(p - 5);
            else pack2(ns, p - 13);
        };
        // one k-step: multiply operand set `set`, prepare set ^ 1 from (slab, kk).  parc >= 0: the slab switch happens inside - this is the second step of a
        // slab of absolute parity parc, `slab` is the next one and `refill` the slab that takes the stage the current one leaves
        auto step = [&](auto setc, uint32_t slab, auto kkc, auto parc, uint32_t refill) __attribute__((always_inline)) {
            constexpr int set = decltype(setc)::value, kk = decltype(kkc)::value, par = decltype(parc)::value;
            constexpr bool boundary = par >= 0;
            constexpr int ns_par = par ^ 1;                         // absolute parity of `slab` (boundary)
            constexpr int ns = set ^ 1;
            constexpr int q0 = boundary ? BQ : 0;                   // first MFMA that has preparation work behind it
            constexpr int vs = 4;                                   // vector work starts this many slots after the weight read
            constexpr int nslots = NMF - q0 - vs;
            static_assert(NMF - BQ >= NDS && NMF - BQ - vs >= 1 && NMF - BQ - 1 >= 4, "the boundary step holds every read and every DMA");
#pragma unroll
            for (int q = 0; q < NMF; ++q) {
                if (boundary && q == q0) {
                    if (pair_wave) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(gemm_q41_pending(NST - 2, par & 1, true)) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(gemm_q41_pending(NST - 2, par & 1, false)) : "memory");
                    barrier_lds_only();         // (+ lgkmcnt(0): this wave's own reads of the slab and its pair are complete before anybody's DMA may overwrite them)
                    __builtin_amdgcn_sched_barrier(0);
                }
                mfma_q(set, q);
                const int e = q - q0;
                if (e >= 0) {
                    if (e == 0) { if (boundary) read_w(slab); }
                    else if (e == 1) { if (boundary && ns_par == 0) read_pm(slab); }
                    else if (e < NDS) read_x(ns, slab, kk, (e - 2) / TN, (e - 2) % TN);
                    if (boundary && e >= 1 && e - 1 < 4) issue1(refill, e - 1, ((par + NST) & 1) == 0);
                    if (e == vs && boundary) set_dm(ns_par != 0);
                    if (e >= vs) {
                        const int s = e - vs;
#pragma unroll
                        for (int p = s * NPC / nslots; p < (s + 1) * NPC / nslots; ++p) piece(ns, kk, p);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        using c0 = std::integral_constant<int, 0>; using c1 = std::integral_constant<int, 1>;
        auto slab_body = [&](uint32_t kt, auto parc) __attribute__((always_inline)) {
            step(c0{}, kt, c1{}, std::integral_constant<int, -1>{}, 0);         // first step of slab kt; prepares its second step
            step(c1{}, kt + 1 < nk ? kt + 1 : kt, c0{}, parc, kt + NST);        // second step; prepares the first step of slab kt + 1
        };
        // prologue: slabs 0 .. NST - 1; slab 0 brings its pair whatever its parity
#pragma unroll
        for (int j = 0; j < NST; ++j) {
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) issue1((uint32_t)j, pc, j == 0 || ((odd + (uint32_t)j) & 1u) == 0);
        }
        if (pair_wave) {                                                        // slab 0 of mine
            if (odd) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(gemm_q41_pending(NST - 1, 0, true)) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(gemm_q41_pending(NST - 1, 1, true)) : "memory");
        } else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(gemm_q41_pending(NST - 1, 0, false)) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        read_w(0);
        read_pm(0);
        set_dm(odd != 0);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int i = 0; i < TN; ++i) read_x(0, 0, 0, pl, i);
#pragma unroll
        for (int p = 0; p < NPC; ++p) piece(0, 0, p);
        __builtin_amdgcn_sched_barrier(0);
        uint32_t kt = 0;
        if (odd) { slab_body(0, c1{}); kt = 1; }
        for (; kt + 1 < nk; kt += 2) {
            slab_body(kt, c0{});
            slab_body(kt + 1, c1{});
        }
        if (kt < nk) slab_body(kt, c0{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the redundant tail DMA
        float* Y = splits > 1 ? a.part + ((size_t)(g * splits + ks) * a.N) * a.M : a.y[g];
        const float* R = splits > 1 ? nullptr : a.r[g];
        if (splits > 1) gemm_store<TN, TM>(a, acc, Y, R, n0, m0 + (uint32_t)wave * 32, li, lh, a.M);
        else if (a.epi != GEMM_EPI_STORE) gemm_store_fused<TN, TM>(a, acc, g, n0, m0 + (uint32_t)wave * 32, li, lh);
        else gemm_store<TN, TM>(a, acc, Y, R, n0, m0 + (uint32_t)wave * 32, li, lh, a.ldy);
    }
}

}  // namespace lh
