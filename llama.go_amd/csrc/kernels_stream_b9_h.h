// csrc/kernels_stream_b9_h.h — k_stream_b9_h: k_stream_b9 (kernels_stream_b9.h) over a weight matrix kept f16 in HBM (dtype 1; DESIGN 3k "Native planes
// kernel"): 49..64 token rows per weight pass of an f16 model, read from the halves.
//     Y_g[c][m] (+ R_g[c][m]) = sum_k X[c][k] * float(W_g[m][k])
// The fp32 kernel over the widened matrix issues eight bf16 products per (column tile, weight tile) and k-block, in the order
//     (xl,wm) (xm,wl) (xl,wh) (xm,wm) (xh,wl) (xm,wh) (xh,wm) (xh,wh).
// A widened half has at most 11 significant bits: its third bf16 part is +0 for every finite half (gemm_f16_layout.h, tests/test_f16_tiles_cpu.py).  The
// two MFMAs that read wl add exact zeros to an accumulator that started at +0 and never holds -0, so every accumulator keeps its value: leaving them out
// (NPROD = 6) leaves each accumulator's sequence of non-zero additions as it was.  NPROD = 8 issues the two with a zero operand in their places.
//
// Kept from k_stream_b9, i.e. everything that decides which products meet in which accumulator in which order: 512 threads as four loader waves (nothing
// but `buffer_load_dwordx4 ... lds`) and four MFMA waves (never touch global memory), one workgroup barrier per 64-column chunk with the MFMA waves one
// chunk behind the ring, MFMA wave = (k-block of 32 columns, half the tiles x all column tiles | CSP: every tile x half the column tiles), the tile / pair
// / K-split deal (t0, nt, ks, ch0, nch), the three activation planes with layout and swizzle, StreamArgs, the stream_epilogue calls.  kernels_stream_b9.h
// stays as it is; the loop is restated because its weight side differs -
//   * the weight image holds halves, [MAXT * 16 rows][64 halves], 128-byte rows: a plane's geometry, swizzle and ds_read_b128 pattern
//     (stream_b9h_layout.h).  A lane's 8 halves of a k-block are ONE LDS read (fp32: two); a 1 KB DMA instruction covers 8 weight rows of one tile;
//   * an image is MAXT * 2048 + NCT * 6144 bytes (36 KB at (6, 4), fp32: 48): as many as fit, up to four.  The ring depth is not part of the sums;
//   * a fragment is split as k_gemm_b9_h splits it (gemm_h_split: v_cvt_f32_f16 with f16 denormals kept, r1 = w - (w & 0xffff0000)) and the high halves
//     of w and r1 packed with k_stream_b9's byte-permute: 8 x 3 + 8 = 32 vector instructions per fragment (fp32: 44), no lo register;
//   * 6 NCW MFMAs per tile with the preparation work rebalanced behind them (S0, NPC, eight moves of `spare`).
//
// Addresses.  Planes: k_stream_b9's (row >= n -> n - 1, chunk past nch -> nch - 1).  Weights: a tile slot past nt becomes slot nt - 1, so the virtual
// tile is t0 + ts < t1 <= the launch's tile count and (matrix g, tile) names a 16-row tile of one of the a.groups matrices: weight row tile * 16 + (r & 15)
// <= M - 1, at byte (row * K) * 2 of a matrix of pitch 2 K bytes.  The chunk is ch0 + min(ch, nch - 1) <= K / 64 - 1 and the source granule <= 7, so the
// column offset is at most (K / 64 - 1) * 128 + 112 bytes and the 16 bytes fetched end at 2 K bytes of the row: every DMA reads inside [M][K] x 2 bytes.
// LDS: piece q < pieces, lane i writes [dst(q), + 16) inside the image (b9h_piece).
// Values: the contract of kernels_gemm_b9.h.  Every finite half, subnormals included, widens to 0 or a magnitude >= 2^-24 with parts >= 2^-24: inside it.
// An infinite or NaN half is outside it, as an infinite fp32 weight is.
#pragma once
#include "kernels_stream_b9.h"
#include "gemm_f16_layout.h"
#include "stream_b9h_layout.h"

namespace lh {

#ifndef B9SH_NIMG_CAP
#define B9SH_NIMG_CAP 4   // probe builds: the ring depth (unmeasured below four)
#endif

template <int MAXT, int NCT, int NIMG, int NPROD = 6, bool CSP = stream_b9_csp(MAXT, NCT)>
__global__ __launch_bounds__(B9S_TH) void k_stream_b9_h(const StreamArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.r[2], a.epi, a.gamma, a.ys_plane, a.ldys);   // the argument block's lines behind one wait (kernels_common.h)
    constexpr int KC = B9S_KC;
    static_assert(NIMG >= 2 && NIMG <= 5, "ring");
    static_assert(NCT >= 1 && NCT <= 4, "column tiles");
    static_assert(NPROD == 8 || NPROD == 6, "products");
    constexpr int XR = NCT * 16;                // staged activation rows per plane
    constexpr int NI = (int)b9h_pieces(MAXT, NCT);
    constexpr int NIW = (NI + 3) / 4;           // DMA instructions per loader wave and chunk
    constexpr int WAITN = NIW * (NIMG - 2) < 64 ? NIW * (NIMG - 2) : 63;
    constexpr uint32_t W_BYTES = b9h_w_bytes(MAXT), XP_BYTES = b9h_plane_bytes(NCT), IMG_BYTES = b9h_image_bytes(MAXT, NCT);
    static_assert(!CSP || NCT % 2 == 0, "column halves");
    static_assert((size_t)NIMG * IMG_BYTES / 4 / ((size_t)2 * XR * 16) >= 2, "stream_epilogue needs room for a tile pair in the dead images");
    constexpr int T0 = CSP ? MAXT : (MAXT + 1) / 2, TPW = T0;   // tiles of part 0 = tile slots of an MFMA wave
    constexpr int NCW = CSP ? NCT / 2 : NCT;    // column tiles of an MFMA wave
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles_per_mat = a.M >> 4, T = tiles_per_mat * a.groups;
    const bool pairs = a.epi == ST_EPI_SILU_MUL;   // virtual tile v = (tile v >> 1 of matrix v & 1), dealt in PAIRS (k_stream_mm2)
    const uint32_t units = pairs ? tiles_per_mat : T, um = pairs ? 2u : 1u;
    const uint32_t S = a.ksplit > 1 ? a.ksplit : 1u, bg = (uint32_t)blockIdx.x / S, ks = (uint32_t)blockIdx.x - bg * S, ng = (uint32_t)gridDim.x / S;
    if (bg >= ng) return;
    const uint32_t t0 = um * (bg * units / ng), t1 = um * ((bg + 1) * units / ng);
    if (t1 <= t0) return;
    const uint32_t nt = t1 - t0;                // <= MAXT (host)
    const uint32_t nch_all = a.K / KC, ch0 = ks * nch_all / S;
    const uint32_t nch = (ks + 1) * nch_all / S - ch0;
    const uint32_t kbase = ch0 * KC;
    if (nch == 0) return;
    const uint32_t r16 = (uint32_t)lane & 15, slot = (uint32_t)lane >> 4;
    f4m acc[TPW][NCW];
    if (wave < 4) {
        // ---- loader waves: piece q = 4 j + wave of a chunk (the tiles' weight rows, then the three planes); a piece's lanes sit in ONE 16-row
        // tile / one plane, so its first row is a uniform resource base and the lane keeps (row) * pitch + its swizzled granule
        uint32_t voff[NIW], doff[NIW], sstep[NIW];
        const char* base[NIW];
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            uint32_t q = (uint32_t)j * 4 + (uint32_t)wave;
            q = q < (uint32_t)NI ? q : (uint32_t)NI - 1;                   // surplus slots repeat the last piece (same bytes to the same place)
            const B9hPiece pc = b9h_piece(MAXT, NCT, q, (uint32_t)lane);
            if (pc.kind == 0) {
                uint32_t ts = q >> 1;                                      // tile slot of the instruction: uniform
                ts = ts < nt ? ts : nt - 1;                                // slots beyond the block: a valid tile again, its sums are never stored
                const uint32_t v = t0 + ts;
                uint32_t g, tile;
                if (pairs) { g = v & 1u; tile = v >> 1; }
                else { g = (v >= tiles_per_mat ? 1u : 0u) + (v >= 2 * tiles_per_mat ? 1u : 0u); tile = v - g * tiles_per_mat; }   // (<= 3 matrices: no division)
                // (a.w[] of this kernel name halves: every offset below is formed from K in halves)
                base[j] = (const char*)((const uint16_t*)(g == 0 ? a.w[0] : (g == 1 ? a.w[1] : a.w[2])) + (size_t)tile * 16 * a.K + kbase);
                voff[j] = ((pc.row & 15u) * a.K + pc.gran * 8u) * 2u;
            } else {
                const uint32_t c = pc.row < a.n ? pc.row : a.n - 1;        // rows past the batch: the last row again (never stored)
                base[j] = (const char*)(a.xs + (size_t)(pc.kind - 1u) * a.xs_plane + kbase);
                voff[j] = (c * a.ldxs + pc.gran * 8u) * 2u;
            }
            sstep[j] = KC * 2;                                             // halves and bf16: 128 bytes per chunk on both sides
            doff[j] = b9h_piece(MAXT, NCT, q, 0u).dst;                     // the instruction's base (lane 0's bytes): uniform
        }
        auto issue = [&](uint32_t ch) {
            const uint32_t cc = ch < nch ? ch : nch - 1;                   // past the end: a harmless reload into a free image (uniform counts)
            char* im = smem_raw + (size_t)(ch % NIMG) * IMG_BYTES;
            // (resource and destination as named locals: kernels_stream.h, k_stream_dma)
#pragma unroll
            for (int j = 0; j < NIW; ++j) {     // 1 KB per instruction
                const __amdgpu_buffer_rsrc_t rs = stream_rsrc(base[j]);
                __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(im + doff[j]);
                const int so = (int)(cc * sstep[j]);
                if (doff[j] < W_BYTES) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, (int)voff[j], so, 0, 2);   // weights: read once (nt)
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, (int)voff[j], so, 0, 0);                     // planes: every workgroup reads them, out of L2
            }
        };
#pragma unroll
        for (int c = 0; c < NIMG - 1; ++c) issue((uint32_t)c);
        for (uint32_t ch = 0; ch < nch; ++ch) {
            wait_vm<WAITN>();                   // chunk ch of this wave has landed; the NIMG - 2 younger ones may still be in flight
            __builtin_amdgcn_s_barrier();       // barrier ch: every part of chunk ch is in its image, and the MFMA waves have left chunk ch - 1's
            issue(ch + NIMG - 1);               // ... whose image takes chunk ch + NIMG - 1
        }
        __builtin_amdgcn_s_barrier();           // the MFMA waves' extra period (the last chunk's MFMAs)
        wait_vm<0>();                           // the clamped tail requests
    } else {
        // ---- MFMA waves
        const uint32_t cw = (uint32_t)(wave - 4), kb = cw >> 1, part = cw & 1u, tb = CSP ? 0u : part * T0, cb = CSP ? part * NCW : 0u;
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int c = 0; c < NCW; ++c) acc[j][c] = f4m{0.f, 0.f, 0.f, 0.f};
        uint32_t woff[TPW], xoff[NCW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            uint32_t t = tb + (uint32_t)j;
            t = t < (uint32_t)MAXT ? t : (uint32_t)MAXT - 1;               // (part 1 of an odd tile count: its last slot repeats a tile, never stored)
            woff[j] = b9h_w_read_off(t, r16, kb, slot);                    // the whole fragment: one granule
        }
#pragma unroll
        for (int c = 0; c < NCW; ++c) xoff[c] = b9h_x_read_off(MAXT, NCT, 0, cb + (uint32_t)c, r16, kb, slot);
        auto image = [&](uint32_t ch) { return (const char*)(smem_raw + (size_t)(ch % NIMG) * IMG_BYTES); };
        u4 wsp[TPW][2], spare[2];               // this chunk's weight fragments as two bf16 pieces each (hi, mid); the fragment being prepared
        u4 xa[NCW][3], xb[NCW][3];              // two operand sets of the planes, swapped by name
        u4 raw[TPW];                            // the next chunk's fragments as they come out of LDS: 8 halves each
        uint32_t s0[8], s1[8];                  // a fragment's widened values and residuals on their way into `spare`
        // One period, scheduled BY HAND as k_stream_b9's: the operands of chunk ch are in registers (wsp, xc); after every MFMA, fenced by
        // sched_barrier(0), ONE slot of filler work for chunk ch + 1 - whose image was completed a barrier ago:
        //   slots 0 .. NDS - 1 of the period      the TPW + 3 NCW operand reads (fragments first)
        //   tile j's slots from S0 on              fragment j: eight 3-instruction splits (widen, and, subtract), then eight byte-permutes into `spare`
        //                                          (tile j's MFMAs still read wsp[j])
        //   the first four slots of tile j + 1     `spare` -> wsp[j] (behind tile j's last MFMA), two dwords per slot
        // (No branch on "is there a next chunk": behind the last one the reads take whatever the ring's next image holds - the loader's clamped
        // tail requests - and the fragments made of it are never multiplied.)
        constexpr int NMT = NPROD * NCW;                           // MFMAs per tile
        constexpr int NDS = TPW + 3 * NCW;
        constexpr int S0 = NMT >= 24 ? 8 : (NMT >= 12 ? 4 : 2);    // first split slot of a tile (the fragment's way from LDS; the moves of the tile before)
        constexpr int NPC = 16;                                    // pieces per fragment: 8 splits + 8 permutes
        // (`spare` moves out in slots 0..3 of a tile; the tile's first permute stands in slot S0 + 8 (NMT - S0) / 16 or later, and a move stands first in its slot)
        static_assert(NMT >= 6 && S0 + 8 * (NMT - S0) / NPC >= 4, "the first permute stands behind the last move");
        auto ds_slot = [&](int e, const char* im, u4 (&xn)[NCW][3]) {
            if (e < TPW) raw[e] = *(const u4*)(im + woff[e]);
            else {
                const int c = (e - TPW) / 3, pl = (e - TPW) % 3;
                xn[c][pl] = *(const u4*)(im + xoff[c] + (size_t)pl * XP_BYTES);
            }
        };
        auto split_f = [&](int j, int f) {      // 3 vector instructions
            const uint32_t d = raw[j][f >> 1];
            gemm_h_split((uint16_t)((f & 1) ? d >> 16 : d & 0xffffu), &s0[f], &s1[f]);
            asm volatile("" : "+v"(s0[f]), "+v"(s1[f]));   // (an empty asm that "uses" the results: without it the optimiser sinks the arithmetic out of its slot, below the fences)
        };
        auto pack1 = [&](int k) {               // one byte-permute: dword k & 3 of part k >> 2
            const int pl = k >> 2, d = k & 3;
            spare[pl][d] = pl == 0 ? __builtin_amdgcn_perm(s0[2 * d + 1], s0[2 * d], 0x07060302u) : __builtin_amdgcn_perm(s1[2 * d + 1], s1[2 * d], 0x07060302u);
            asm volatile("" : "+v"(spare[pl]));
        };
        auto period = [&](uint32_t ch, const u4 (&xc)[NCW][3], u4 (&xn)[NCW][3]) {
            const char* im = image(ch + 1);
            const u4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
#pragma unroll
                for (int m = 0; m < NMT; ++m) {
                    const int q = m / NCW, c = m % NCW, e = j * NMT + m;
                    const int px = b9h_product_x(NPROD, q), pw = b9h_product_w(NPROD, q);
                    acc[j][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xc[c][px]), __builtin_bit_cast(bf16x8, pw == 2 ? zero : wsp[j][pw & 1]), acc[j][c], 0, 0, 0);
                    if (e < NDS) ds_slot(e, im, xn);
                    else if (NDS > NMT * TPW && m == NMT - 1 && j == TPW - 1) {   // (fewer MFMAs than reads: the rest behind the last one)
#pragma unroll
                        for (int r = NMT * TPW; r < NDS; ++r) ds_slot(r, im, xn);
                    }
                    if (j > 0 && m < 4) {                                  // tile j - 1's fragment into place, two dwords per slot
                        const int k0 = 2 * m;
                        wsp[j - 1][k0 >> 2][k0 & 3] = spare[k0 >> 2][k0 & 3]; wsp[j - 1][k0 >> 2][(k0 & 3) + 1] = spare[k0 >> 2][(k0 & 3) + 1];
                        asm volatile("" : "+v"(wsp[j - 1][k0 >> 2]));
                    }
                    if (m >= S0) {
                        const int sl = m - S0, nsl = NMT - S0;
#pragma unroll
                        for (int pc = sl * NPC / nsl; pc < (sl + 1) * NPC / nsl; ++pc) {
                            if (pc < 8) split_f(j, pc);
                            else pack1(pc - 8);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) wsp[TPW - 1][pl] = spare[pl];   // the last tile's fragment (behind its last MFMA)
            __builtin_amdgcn_sched_barrier(0);
        };
        barrier_lds_only();                     // barrier 0: chunk 0 is in image 0
#pragma unroll
        for (int e = 0; e < NDS; ++e) ds_slot(e, smem_raw, xa);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
#pragma unroll
            for (int f = 0; f < 8; ++f) split_f(j, f);
#pragma unroll
            for (int k = 0; k < 8; ++k) pack1(k);
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) wsp[j][pl] = spare[pl];
        }
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t ch = 0; ch < nch; ch += 2) {   // two chunks per trip: the operand sets swap by name
            barrier_lds_only();                 // barrier ch + 1
            period(ch, xa, xb);
            if (ch + 1 < nch) {
                barrier_lds_only();             // barrier ch + 2
                period(ch + 1, xb, xa);
            }
        }
    }
    __syncthreads();   // the images are dead (the loader waves have drained their DMAs: a pending LDS-DMA would land in `part`)
    if constexpr (CSP) stream_epilogue<MAXT, NCT, 2, true>(a, smem_raw, (uint32_t)((size_t)NIMG * IMG_BYTES / 4), nullptr, t0, nt, ks, tiles_per_mat, [&](int t, int c) { return acc[t][c]; });
    else stream_epilogue<MAXT, NCT, 1, true, 0, 2>(a, smem_raw, (uint32_t)((size_t)NIMG * IMG_BYTES / 4), nullptr, t0, nt, ks, tiles_per_mat,
                                                   [&](int t, int c) { return acc[t >= T0 ? t - T0 : t][c]; });
}

}  // namespace lh
