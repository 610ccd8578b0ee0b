// csrc/kernels_stream_b9w_h.h — k_stream_b9w_h: k_stream_b9w (kernels_stream_b9w.h) over a weight matrix kept f16 in HBM (dtype 1; DESIGN 3k "Native wide
// planes kernel"), as k_stream_b9_h is to k_stream_b9: 65..128 token rows of ONE weight pass of an f16 model, read from the halves.
//     Y_g[c][m] (+ R_g[c][m]) = sum_k X[c][k] * float(W_g[m][k])
// Opt-in: lh_ctx_set_f16_planes AND lh_ctx_set_wide_planes (plan.hip, eval_planes).
// The fp32 kernel over the widened matrix issues eight bf16 products per (column tile, weight tile) and k-block, in the order
//     (xl,wm) (xm,wl) (xl,wh) (xm,wm) (xh,wl) (xm,wh) (xh,wm) (xh,wh).
// A widened half has at most 11 significant bits: its third bf16 part is +0 for every finite half (gemm_f16_layout.h, tests/test_f16_tiles_cpu.py).  The
// two MFMAs that read wl add products (finite x) * (+0) = +-0 to the accumulator.  An accumulator starts at +0 and never holds -0: a sum is -0 only when
// both terms are, and by induction no term that enters is added to a -0.  Adding +-0 to +0 gives +0 and to a non-zero value gives that value, so the two
// MFMAs leave every accumulator's bytes as they were: leaving them out (NPROD = 6, the products b9h_product_x / b9h_product_w give, in the same relative
// order) leaves each accumulator's sequence of non-zero additions as it was.  NPROD = 8 (-DB9WH_PRODUCTS=8) issues the two with a zero operand in their places.
//
// Kept from k_stream_b9w, i.e. everything that decides which products meet in which accumulator in which order: the three activation planes with layout
// and swizzle, StreamArgs, the tile / pair / K-split deal (t0, nt, ks, ch0, nch), four loader waves that only issue `buffer_load_dwordx4 ... lds` against
// counted vmcnt waits, four MFMA waves as 2 k-blocks x 2 column halves, each holding all MAXT row tiles next to b9w_ncw(NCT) column tiles, b9w_col_tile's
// repeated slot for an odd column-tile count, one workgroup barrier per 64-column chunk with the first fragment and the operand set read behind it, the
// stream_epilogue<MAXT, NCE, 2, true> call.  kernels_stream_b9w.h stays as it is; the loop is restated because its weight side differs -
//   * the weight image holds halves, [MAXT * 16 rows][64 halves] in 128-byte rows (stream_b9wh_layout.h: stream_b9h_layout.h's geometry, swizzle and 1 KB
//     pieces of eight weight rows of one tile); a.w[] name halves and every weight offset is formed from K in halves;
//   * an image is MAXT * 2048 + NCT * 6144 bytes (64 KB at (8, 8), fp32: 80): as many as fit 160 KB, up to four (b9wh_nimg; three at (6, 6), where fp32
//     fits two).  The ring depth is not part of the sums;
//   * tile j + 1's fragment is ONE ds_read_b128 (slot 0 of tile j), split as k_stream_b9_h splits it (gemm_h_split: v_cvt_f32_f16 with f16 denormals
//     kept, mask, one exact subtraction) and packed by eight byte-permutes into two bf16 pieces (hi, mid): 8 x 3 + 8 = 32 vector instructions as 16 pieces
//     of work (fp32: 44 as 20), no lo piece; the two buffers wa[2] / wb[2] swap by name;
//   * 6 NCW = 18 or 24 MFMAs per tile (fp32: 24 or 32) with the sixteen pieces rebalanced behind them: S0 = 4 (18) | 6 (24 and more) leaves the read four
//     to five MFMAs on its way from LDS and at most two pieces in a slot, every slot fenced by sched_barrier(0).
//
// Addresses.  Planes: k_stream_b9w's (row >= n -> n - 1, chunk past nch -> nch - 1).  Weights: a tile slot past nt becomes slot nt - 1, so the virtual
// tile is t0 + ts < t1 <= the launch's tile count and (matrix g, tile) names a 16-row tile of one of the a.groups matrices: weight row tile * 16 + (r & 15)
// <= M - 1, at byte (row * K) * 2 of a matrix of pitch 2 K bytes.  The chunk is ch0 + min(ch, nch - 1) <= K / 64 - 1 and the source granule <= 7, so the
// column offset is at most (K / 64 - 1) * 128 + 112 bytes and the 16 bytes fetched end at 2 K bytes of the row: every DMA reads inside [M][K] x 2 bytes.
// LDS: piece q < pieces, lane i writes [dst(q) + 16 i, + 16) inside the image (b9wh_piece); a fragment read ends at tile slot MAXT - 1's last row.
// Values: the contract of kernels_gemm_b9.h.  Every finite half, subnormals included, widens to 0 or a magnitude >= 2^-24 with parts >= 2^-24: inside it.
// An infinite or NaN half is outside it, as an infinite fp32 weight is.
#pragma once
#include "kernels_stream_b9.h"
#include "gemm_f16_layout.h"
#include "stream_b9wh_layout.h"

namespace lh {

template <int MAXT, int NCT, int NIMG, int NPROD = 6>
__global__ __launch_bounds__(B9S_TH) void k_stream_b9w_h(const StreamArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.r[2], a.epi, a.gamma, a.ys_plane, a.ldys);   // the argument block's lines behind one wait (kernels_common.h)
    constexpr int KC = B9S_KC;
    static_assert(b9wh_built(MAXT, NCT), "row tiles x column tiles");
    static_assert(NIMG >= 2 && NIMG <= 4 && (uint32_t)NIMG * b9wh_image_bytes(MAXT, NCT) <= B9W_LDS_BYTES, "ring");
    static_assert(NPROD == 8 || NPROD == 6, "products");
    constexpr int NCW = (int)b9w_ncw(NCT), NCE = 2 * NCW;   // column tiles of an MFMA wave; of the epilogue (even)
    constexpr int NWI = 2 * MAXT, NI = (int)b9wh_pieces(MAXT, NCT);
    constexpr int NIW = (NI + 3) / 4;           // DMA instructions per loader wave and chunk
    constexpr int WAITN = NIW * (NIMG - 2) < 64 ? NIW * (NIMG - 2) : 63;
    constexpr uint32_t W_BYTES = b9wh_w_bytes(MAXT), XP_BYTES = b9wh_plane_bytes(NCT), IMG_BYTES = b9wh_image_bytes(MAXT, NCT);
    static_assert((size_t)NIMG * IMG_BYTES / 4 / ((size_t)2 * NCE * 16 * 16) >= 2, "stream_epilogue needs room for a tile pair in the dead images");
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
    f4m acc[MAXT][NCW];
    if (wave < 4) {
        // ---- loader waves: piece q = 4 j + wave of a chunk (stream_b9wh_layout.h).  A piece's lanes sit in ONE 16-row tile / one plane, so its first
        // row is a uniform resource base and the lane keeps (row) * pitch + the source granule of the position it lands on
        uint32_t voff[NIW], doff[NIW];
        const char* base[NIW];
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            uint32_t q = (uint32_t)j * 4 + (uint32_t)wave;
            q = q < (uint32_t)NI ? q : (uint32_t)NI - 1;                   // surplus slots repeat the last piece (same bytes to the same place)
            const B9hPiece p0 = b9wh_piece(MAXT, NCT, q, 0), pl = b9wh_piece(MAXT, NCT, q, (uint32_t)lane);   // uniform part; this lane's row and granule
            doff[j] = p0.dst;
            if (q < (uint32_t)NWI) {
                uint32_t ts = q >> 1;                                      // tile slot of the piece: uniform
                ts = ts < nt ? ts : nt - 1;                                // slots beyond the block: a valid tile again, its sums are never stored
                const uint32_t v = t0 + ts;
                uint32_t g, tile;
                if (pairs) { g = v & 1u; tile = v >> 1; }
                else { g = (v >= tiles_per_mat ? 1u : 0u) + (v >= 2 * tiles_per_mat ? 1u : 0u); tile = v - g * tiles_per_mat; }   // (<= 3 matrices: no division)
                // (a.w[] of this kernel name halves: every offset below is formed from K in halves)
                base[j] = (const char*)((const uint16_t*)(g == 0 ? a.w[0] : (g == 1 ? a.w[1] : a.w[2])) + (size_t)tile * 16 * a.K + kbase);
                voff[j] = ((pl.row & 15u) * a.K + pl.gran * 8u) * 2u;
            } else {
                const uint32_t c = pl.row < a.n ? pl.row : a.n - 1;        // rows past the batch: the last row again (never stored)
                base[j] = (const char*)(a.xs + (size_t)(p0.kind - 1u) * a.xs_plane + kbase);
                voff[j] = (c * a.ldxs + pl.gran * 8u) * 2u;
            }
        }
        auto issue = [&](uint32_t ch) {
            const uint32_t cc = ch < nch ? ch : nch - 1;                   // past the end: a harmless reload into a free image (uniform counts)
            char* im = smem_raw + (size_t)(ch % NIMG) * IMG_BYTES;
            const int so = (int)(cc * (KC * 2));                           // halves and bf16: 128 bytes per chunk on both sides
            // (resource and destination as named locals: kernels_stream.h, k_stream_dma)
#pragma unroll
            for (int j = 0; j < NIW; ++j) {     // 1 KB per instruction
                const __amdgpu_buffer_rsrc_t rs = stream_rsrc(base[j]);
                __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(im + doff[j]);
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
        wait_vm<0>();                           // the clamped tail requests
    } else {
        // ---- MFMA waves: wave 4 + 2 kb + half
        const uint32_t cw = (uint32_t)(wave - 4), kb = cw >> 1, half = cw & 1u;
#pragma unroll
        for (int j = 0; j < MAXT; ++j)
#pragma unroll
            for (int c = 0; c < NCW; ++c) acc[j][c] = f4m{0.f, 0.f, 0.f, 0.f};
        const uint32_t woff = b9wh_w_read_off(0, r16, kb, slot);           // tile slot j: + 2048 j; the whole fragment is one granule
        uint32_t xoff[NCW];
#pragma unroll
        for (int c = 0; c < NCW; ++c) xoff[c] = b9wh_x_read_off(MAXT, NCT, 0, b9w_col_tile(NCT, half, (uint32_t)c), r16, kb, slot);   // plane p: + p XP_BYTES
        u4 xc[NCW][3];                          // this chunk's operands of the wave's column tiles
        u4 wa[2], wb[2];                        // two weight fragments as two bf16 pieces each (hi, mid), swapped by name
        u4 raw;                                 // a fragment as it comes out of LDS: 8 halves
        uint32_t s0[8], s1[8];                  // its widened values and residuals on their way into the pieces
        constexpr int NMT = NPROD * NCW;        // MFMAs per tile
        constexpr int S0 = NMT >= 24 ? 6 : 4;   // first split slot of a tile (the fragment's way from LDS)
        constexpr int NPC = 16;                 // pieces per fragment: 8 splits + 8 permutes
        static_assert(S0 >= 1 && S0 < NMT && b9wh_pieces_issued(NMT, S0, NPC) == NPC, "no piece of a fragment is left over");
        auto read_w = [&](const char* im, int j) { raw = *(const u4*)(im + woff + (uint32_t)j * 2048u); };
        auto split_f = [&](int f) {             // 3 vector instructions
            const uint32_t d = raw[f >> 1];
            gemm_h_split((uint16_t)((f & 1) ? d >> 16 : d & 0xffffu), &s0[f], &s1[f]);
            asm volatile("" : "+v"(s0[f]), "+v"(s1[f]));   // (keeps the arithmetic in its slot: kernels_stream_b9.h)
        };
        auto pack1 = [&](u4 (&w)[2], int k) {   // one byte-permute: dword k & 3 of piece k >> 2
            const int pl = k >> 2, d = k & 3;
            w[pl][d] = pl == 0 ? __builtin_amdgcn_perm(s0[2 * d + 1], s0[2 * d], 0x07060302u) : __builtin_amdgcn_perm(s1[2 * d + 1], s1[2 * d], 0x07060302u);
            asm volatile("" : "+v"(w[pl]));
        };
        // tile j's MFMAs out of `wc`, tile j + 1's fragment on its way into `wn`: the read in slot 0, the sixteen pieces from slot S0 on
        auto tile = [&](const char* im, int j, const u4 (&wc)[2], u4 (&wn)[2]) {
            const u4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int m = 0; m < NMT; ++m) {
                const int q = m / NCW, c = m % NCW;
                const int px = b9h_product_x(NPROD, q), pw = b9h_product_w(NPROD, q);
                acc[j][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xc[c][px]), __builtin_bit_cast(bf16x8, pw == 2 ? zero : wc[pw & 1]), acc[j][c], 0, 0, 0);
                if (j + 1 < MAXT) {
                    if (m == 0) read_w(im, j + 1);
                    if (m >= S0) {
                        const int sl = m - S0, nsl = NMT - S0;
#pragma unroll
                        for (int pc = sl * NPC / nsl; pc < (sl + 1) * NPC / nsl; ++pc) {
                            if (pc < 8) split_f(pc);
                            else pack1(wn, pc - 8);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (uint32_t ch = 0; ch < nch; ++ch) {
            barrier_lds_only();                 // barrier ch: chunk ch is in its image (this wave's reads of chunk ch - 1 are complete: lgkmcnt(0))
            const char* im = smem_raw + (size_t)(ch % NIMG) * IMG_BYTES;
            read_w(im, 0);
#pragma unroll
            for (int c = 0; c < NCW; ++c)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) xc[c][pl] = *(const u4*)(im + xoff[c] + (size_t)pl * XP_BYTES);
#pragma unroll
            for (int f = 0; f < 8; ++f) split_f(f);
#pragma unroll
            for (int k = 0; k < 8; ++k) pack1(wa, k);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MAXT; ++j) {
                if (j & 1) tile(im, j, wb, wa);
                else tile(im, j, wa, wb);
            }
        }
    }
    __syncthreads();   // the images are dead (the loader waves have drained their DMAs: a pending LDS-DMA would land in `part`)
    stream_epilogue<MAXT, NCE, 2, true>(a, smem_raw, (uint32_t)((size_t)NIMG * IMG_BYTES / 4), nullptr, t0, nt, ks, tiles_per_mat, [&](int t, int c) { return acc[t][c]; });
}

}  // namespace lh
