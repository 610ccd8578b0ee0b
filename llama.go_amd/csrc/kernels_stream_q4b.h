// csrc/kernels_stream_q4b.h — k_stream_q8b (kernels_stream_q8b.h) on the 4-bit weights of a block-int4 model as they lie in HBM: no int8 image in between.
//
// Reference: the matmul is ComputeForwardMulMatFP32 (pkg/ml/ml.go:1976-2098); the quantised dtype is ours (format: kernels_q4.h).
//
// Why: a block-int4 model read its nibbles only on the decode stream of one to four rows; every other row count expanded each matrix of each layer into an
// int8 image (k_expand_q4: 0.5 B read + 1 B written per weight) that k_stream_q8b then read (1 B) - 2.5 B per weight where the int8 model moves 1.
// A 4-bit quant n - 8 in [-8, 7] is an exact bf16 like any int8 quant, and a dtype-2 buffer's scale plane has the int8 buffer's shape.  So this kernel differs
// from k_stream_q8b ONLY in where a lane's eight quants come from, and feeds identical operands into the identical MFMA and fma sequence: every sum is the
// int8 twin's bit for bit.
//
// The same (these decide the bits; not restated, see kernels_stream_q8b.h): sixteen equal waves; wave w owns quant block w % NB for the tiles w / NB (mod TG);
// the tile range t0..t1 and the chunk range of a K-split; one workgroup barrier per chunk; the transposed MFMA (A = activation planes, B = weights); planes in
// the order lo, mid, hi; one fmaf(d, block_sum, acc) per output element and block; stream_epilogue<MAXT, NCT, 1, true, NB>; the scale pieces and the three
// activation planes of the image with their layouts and DMA pieces.
// Different:
//   * a weight row of a chunk is KC / 2 bytes of the nibble plane: KC / 32 granules of 16 bytes (ONE granule = one quant block), so 16 / 8 / 4 rows per
//     `buffer_load_dwordx4 ... lds` instruction (KC = 128 / 256 / 512) and a weight part half as large;
//   * the swizzle and the lane's 4-byte operand read: stream_q4_layout.h (one pure function for the DMA side and the reading side);
//   * nibbles -> bf16: stream_q4_operand (same header) - mask-in-place into an fp32 mantissa, one exact subtraction, v_perm_b32 packs two high halves.
//   * NIMG is this kernel's own (the ring depth is no part of the sums): plan.hip, launch_stream_q8b.
#pragma once
#include "kernels_stream_q8b.h"
#include "stream_q4_layout.h"

namespace lh {

__host__ __device__ constexpr size_t stream_q4b_image_bytes(int maxt, int xr, int kc) { return (size_t)maxt * 16 * (kc / 2) + (size_t)maxt * (kc / 32) * 64 + (size_t)3 * xr * kc * 2; }

template <int MAXT, int NCT, int KC, int NIMG, int XR, int TH = Q8B_TH>
__global__ __launch_bounds__(TH) void k_stream_q4b(const StreamArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.r[2], a.epi, a.gamma, a.ys_plane, a.ldys);   // the argument block's lines behind one wait (kernels_common.h)
    static_assert(KC == 128 || KC == 256 || KC == 512, "chunk");
    static_assert(NIMG >= 2 && NIMG <= 4, "ring");
    static_assert(XR == NCT * 16 || (NCT == 1 && XR == 8), "staged activation rows");
    constexpr int NWV = TH / 64;                // waves
    static_assert(NWV >= KC / 32 && NWV % (KC / 32) == 0, "every quant block of a chunk needs its wave(s)");
    constexpr int NB = KC / 32;                 // quant blocks per chunk: 4 / 8 / 16
    constexpr int TG = NWV / NB;                // tile groups: 4 / 2 / 1
    constexpr int TPW = (MAXT + TG - 1) / TG;   // tiles per wave
    constexpr int GRW = KC / 32;                // 16-byte granules per weight row: 4 / 8 / 16 (one per quant block)
    constexpr int RPW = 64 / GRW;               // weight rows per DMA instruction: 16 / 8 / 4
    constexpr int GRX = KC / 8;                 // granules per plane row: 16 / 32 / 64
    constexpr int RPX = 64 / GRX;               // plane rows per DMA instruction: 4 / 2 / 1
    constexpr int NWI = MAXT * 16 / RPW, NSI = MAXT, NXP = XR / RPX, NXI = 3 * NXP, NI = NWI + NSI + NXI;
    constexpr int NIW = (NI + NWV - 1) / NWV;   // DMA instructions per wave and chunk
    constexpr int WAITN = NIW * (NIMG - 2) < 64 ? NIW * (NIMG - 2) : 63;
    constexpr uint32_t W_BYTES = MAXT * 16 * (KC / 2), S_BYTES = MAXT * NB * 64, XP_BYTES = XR * KC * 2, IMG_BYTES = W_BYTES + S_BYTES + 3 * XP_BYTES;
    static_assert(IMG_BYTES == stream_q4b_image_bytes(MAXT, XR, KC), "the launcher sizes the ring with stream_q4b_image_bytes");
    static_assert(NWI * 1024 == (int)W_BYTES, "the weight pieces cover the weight part exactly");
    static_assert((size_t)NIMG * IMG_BYTES / 4 / ((size_t)NB * NCT * 16 * 16) >= 2, "stream_epilogue needs room for a tile pair in the dead images");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles_per_mat = a.M >> 4, T = tiles_per_mat * a.groups;
    const bool pairs = a.epi == ST_EPI_SILU_MUL;
    const uint32_t units = pairs ? tiles_per_mat : T, um = pairs ? 2u : 1u;
    const uint32_t S = a.ksplit > 1 ? a.ksplit : 1u, bg = (uint32_t)blockIdx.x / S, ks = (uint32_t)blockIdx.x - bg * S, ng = (uint32_t)gridDim.x / S;
    if (bg >= ng) return;
    const uint32_t t0 = um * (bg * units / ng), t1 = um * ((bg + 1) * units / ng);
    if (t1 <= t0) return;
    const uint32_t nt = t1 - t0;
    const uint32_t nch_all = a.K / KC, ch0 = ks * nch_all / S;
    const uint32_t nch = (ks + 1) * nch_all / S - ch0;
    const uint32_t kbase = ch0 * KC;
    if (nch == 0) return;
    const uint32_t r16 = (uint32_t)lane & 15, slot = (uint32_t)lane >> 4;
    const uint32_t Kh = a.K >> 1;               // bytes per row of the nibble plane
    auto xswz = [](uint32_t r) -> uint32_t { return XR == 8 ? ((r & 7u) << 1) : (r & 15u); };   // (k_stream_q8b's plane-row swizzle)
    // ---- this wave's DMA instructions of a chunk: piece q = NWV j + wave (weights, the tiles' scales, the three activation planes)
    const char* base[NIW];
    uint32_t voff[NIW], sstep[NIW], doff[NIW];
    bool narrow[NIW];                                                      // a scale piece (fewer active lanes)
#pragma unroll
    for (int j = 0; j < NIW; ++j) {
        uint32_t q = (uint32_t)j * NWV + (uint32_t)wave;
        q = q < (uint32_t)NI ? q : (uint32_t)NI - 1;                       // surplus slots repeat the last piece (same bytes to the same place)
        auto tile_base = [&](uint32_t ts, bool scales) -> const char* {
            ts = ts < nt ? ts : nt - 1;
            const uint32_t v = t0 + ts;
            uint32_t g, tile;
            if (pairs) { g = v & 1u; tile = v >> 1; }
            else { g = (v >= tiles_per_mat ? 1u : 0u) + (v >= 2 * tiles_per_mat ? 1u : 0u); tile = v - g * tiles_per_mat; }   // (<= 3 matrices: no division)
            if (scales) return (const char*)((g == 0 ? a.ws[0] : (g == 1 ? a.ws[1] : a.ws[2])) + (size_t)tile * 16 * (a.K / 32) + kbase / 32);
            return (const char*)(g == 0 ? a.w[0] : (g == 1 ? a.w[1] : a.w[2])) + (size_t)tile * 16 * Kh + kbase / 2;
        };
        narrow[j] = q >= (uint32_t)NWI && q < (uint32_t)(NWI + NSI);
        if (q < (uint32_t)NWI) {
            // lane i lands at q * 1024 + 16 i = position i % GRW of image row q RPW + i / GRW, and fetches the granule stored there
            const uint32_t rr = q * RPW + (uint32_t)lane / GRW, gd = (uint32_t)lane % GRW, gs = stream_q4_granule_pos(KC, rr, gd);
            base[j] = tile_base((q * RPW) >> 4, false);
            voff[j] = (rr & 15u) * Kh + gs * 16u;
            sstep[j] = KC / 2;
            doff[j] = q * 1024u;
        } else if (q < (uint32_t)(NWI + NSI)) {
            const uint32_t ts = q - NWI;
            constexpr uint32_t LPR = KC / 128;                             // 16-byte pieces per row's scales: 1 / 2 / 4
            const uint32_t l = (uint32_t)lane & (16u * LPR - 1u);          // (lanes past 16 LPR are masked off when the instruction issues)
            base[j] = tile_base(ts, true);
            voff[j] = ((l / LPR) * (a.K / 32) + (l % LPR) * 4u) * 4u;
            sstep[j] = (KC / 32) * 4;
            doff[j] = W_BYTES + ts * (NB * 64u);
        } else {
            const uint32_t xq = q - NWI - NSI, p = xq / NXP, xi = xq - p * NXP;
            const uint32_t rr = xi * RPX + (uint32_t)lane / GRX, gd = (uint32_t)lane % GRX, gs = gd ^ xswz(rr);
            const uint32_t c = rr < a.n ? rr : a.n - 1;
            base[j] = (const char*)(a.xs + (size_t)p * a.xs_plane + kbase);
            voff[j] = (c * a.ldxs + gs * 8u) * 2u;
            sstep[j] = KC * 2;
            doff[j] = W_BYTES + S_BYTES + p * XP_BYTES + xi * 1024u;
        }
    }
    // The DMA is inline asm for k_stream_q8b's reason: through the builtin the compiler sees a store to LDS and drains every chunk in flight in front of
    // this wave's next operand read of the ring.  The waits for these DMAs are the explicit counted ones of the loop.
    typedef int i4v __attribute__((ext_vector_type(4)));
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem_raw;
    auto issue = [&](uint32_t ch) {
        const uint32_t cc = ch;
        const uint32_t im = lds0 + (ch % NIMG) * IMG_BYTES;
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            const uint64_t b = (uint64_t)sgpr_ptr(base[j]);
            const i4v rs = {(int)(uint32_t)b, (int)((uint32_t)(b >> 32) & 0xffffu), 0x7fffffff, 0x00020000};   // raw buffer, stride 0 (stream_rsrc's words)
            const uint32_t m0v = (uint32_t)__builtin_amdgcn_readfirstlane((int)(im + doff[j])), so = (uint32_t)__builtin_amdgcn_readfirstlane((int)(cc * sstep[j]));
            if (narrow[j] && KC < 512) {   // a tile's scales: 16 KC / 128 active lanes
                unsigned long long saved;
                asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %5\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b64 exec, %0"
                             : "=&s"(saved) : "s"(m0v), "v"(voff[j]), "s"(rs), "s"(so), "s"(KC == 128 ? 0xffffull : 0xffffffffull) : "memory", "m0");
            } else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(m0v), "v"(voff[j]), "s"(rs), "s"(so) : "memory", "m0");
        }
    };
#pragma unroll
    for (int c = 0; c < NIMG - 1; ++c) if ((uint32_t)c < nch) issue((uint32_t)c);
    // ---- this wave's share of a chunk: quant block kb for the tiles tg, tg + TG, ...
    const uint32_t kb = (uint32_t)wave % NB, tg = (uint32_t)wave / NB;
    f4m acc[TPW][NCT];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[j][c] = f4m{0.f, 0.f, 0.f, 0.f};
    uint32_t woff[TPW], soff[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        uint32_t t = tg + (uint32_t)j * TG;
        t = t < (uint32_t)MAXT ? t : (uint32_t)MAXT - 1;                   // (a slot past the tiles: the last one again, its sums are never stored)
        woff[j] = stream_q4_read_off(KC, t, r16, kb, slot);
        soff[j] = W_BYTES + t * (NB * 64) + r16 * (NB * 4) + kb * 4;
    }
    uint32_t xoff[NCT];
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        const uint32_t row = XR == 8 ? (r16 & 7u) : (uint32_t)c * 16 + r16;   // (rows 8..15 of a half tile: copies of 0..7, never stored)
        xoff[c] = W_BYTES + S_BYTES + (row * GRX + ((kb * 4 + slot) ^ xswz(row))) * 16;
    }
    for (uint32_t ch = 0; ch < nch; ++ch) {
        const char* im = smem_raw + (size_t)(ch % NIMG) * IMG_BYTES;
        // this wave's pieces of chunk ch have landed; the younger chunks' (min(NIMG - 2, chunks left) of them) may still be in flight
        {
            const uint32_t left = nch - 1 - ch;
            if (left >= (uint32_t)(NIMG - 2)) wait_vm<WAITN>();
            else if (NIMG >= 4 && left == 1) wait_vm<(NIW < 64 ? NIW : 63)>();
            else wait_vm<0>();
        }
        barrier_lds_only();                     // barrier ch: every piece of chunk ch is in its image, and everybody has left chunk ch - 1's ...
        if (ch + NIMG - 1 < nch) issue(ch + NIMG - 1);   // ... which takes chunk ch + NIMG - 1
        u4 xo[3][NCT];
        uint32_t raw[TPW];
        float d[TPW];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int c = 0; c < NCT; ++c) xo[p][c] = *(const u4*)(im + xoff[c] + (size_t)p * XP_BYTES);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            raw[j] = *(const uint32_t*)(im + woff[j]);
            d[j] = *(const float*)(im + soff[j]);
        }
        // nibbles -> the bf16 of n - 8, the operand k_stream_q8b holds for the same quants (stream_q4_layout.h)
        u4 wb[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            uint32_t o[4];
            stream_q4_operand(raw[j], o);
            wb[j] = u4{o[0], o[1], o[2], o[3]};
        }
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            // block sums, small pieces first; the wave's tiles interleaved so that consecutive MFMAs are independent
            f4m ps[TPW];
#pragma unroll
            for (int j = 0; j < TPW; ++j) ps[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xo[2][c]), __builtin_bit_cast(bf16x8, wb[j]), f4m{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) ps[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xo[1][c]), __builtin_bit_cast(bf16x8, wb[j]), ps[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) ps[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xo[0][c]), __builtin_bit_cast(bf16x8, wb[j]), ps[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                acc[j][c][0] = fmaf(d[j], ps[j][0], acc[j][c][0]); acc[j][c][1] = fmaf(d[j], ps[j][1], acc[j][c][1]);
                acc[j][c][2] = fmaf(d[j], ps[j][2], acc[j][c][2]); acc[j][c][3] = fmaf(d[j], ps[j][3], acc[j][c][3]);
            }
        }
    }
    __syncthreads();   // the images are dead
    stream_epilogue<MAXT, NCT, 1, true, NB>(a, smem_raw, (uint32_t)((size_t)NIMG * IMG_BYTES / 4), nullptr, t0, nt, ks, tiles_per_mat, [&](int t, int c) { return acc[t / TG][c]; });
}

}  // namespace lh
