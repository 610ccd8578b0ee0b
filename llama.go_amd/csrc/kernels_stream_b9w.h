// csrc/kernels_stream_b9w.h — fp32 weights, 65..128 token rows of ONE weight pass (five to eight 16-token column tiles), on the bf16 matrix pipe with
// EXACT products: k_stream_b9 (kernels_stream_b9.h) for the band it cannot reach.  Opt-in: lh_ctx_set_wide_planes (plan.hip, eval_planes).
//     Y_g[c][m] (+ R_g[c][m]) = sum_k X[c][k] * W_g[m][k]        (ComputeForwardMulMatFP32, pkg/ml/ml.go:1976-2098)
// The rows are a prompt's tokens (server.Do feeds the prompt as ONE Eval, pkg/server/server.go:185-192).  Today they run on k_stream_dma's fp32-input
// MFMAs, which are bound by the matrix pipe from 33 rows on (header of kernels_stream_b9.h).
//
// What is k_stream_b9's, unchanged: the activations as three bf16 planes written by the producing kernels, fp32 weights in HBM split in registers
// (split_f / pack1 below are split3x8 in slot-sized pieces), the eight products of B9S_PRODUCTS in its order (small terms first), StreamArgs, the tile /
// pair / K-split deal (t0, nt, ks, ch0, nch), four loader waves that only issue `buffer_load_dwordx4 ... lds` against counted vmcnt waits, one workgroup
// barrier per 64-column chunk, and stream_epilogue - the partial tiles meet in wave order, so results are bit-reproducible.
//
// What is its own - why k_stream_b9 cannot be stretched (its MFMA wave keeps a chunk's weight fragments of half the tiles, split, plus two operand
// sets of ALL column tiles in registers: 8 column tiles x 3 planes x 4 registers x 2 sets = 192 registers before the first accumulator):
//   * work split: the four MFMA waves are 2 k-blocks (32 columns of the chunk) x 2 COLUMN HALVES; a wave holds every tile of the workgroup next to
//     ceil(NCT / 2) column tiles: MAXT x 4 accumulator tiles (128 registers at eight row tiles) and ONE operand set of its half of the planes (48).  An
//     odd column-tile count gives the second half a slot that repeats the last column tile (b9w_col_tile); its sums are never emitted.
//   * weight fragments are not kept: tile j + 1's fragment (two ds_read_b128) is read and split (8 x 4 + 12 vector instructions) in the issue slots
//     behind tile j's 8 x NCW MFMAs, one piece per slot, fenced by sched_barrier as in k_stream_b9; two fragment buffers swap by name.  So the split
//     runs under the MFMAs inside a chunk.  Across the chunk edge it does not: with 48 KB of planes per chunk only two images fit next to six or eight
//     row tiles, the next chunk is still in flight while this one multiplies, and the first fragment and the operand set are read behind the barrier
//     (3 NCW + 2 reads and 44 vector instructions exposed per 8 MAXT NCW MFMAs: ~ 5 % at six row tiles).  Both column halves split the same fragments
//     (k_stream_b9's CSP does the same): 44 MAXT vector instructions beside 8 MAXT NCW MFMAs of 16 clocks.
//   * plane bytes: per weight byte a workgroup stages 6 n / (64 MAXT) plane bytes out of L2 (7B w1|w3 at 128 rows: 2.0).  Priced:
//       - row groups x K-slices would cut that by the slice count, but only the plain epilogue can leave partial sums (RoPE and silu * mul need
//         the whole contraction): wo / w2 already run as K-split fours through k_stream_reduce_norm (MAXT 4 over a quarter of K: 0.75 at 128 rows),
//         wq|wk|wv and w1|w3 cannot - dropped for them, kept as it stands for wo / w2;
//       - a 32-column chunk halves the image (a third and fourth image) but moves no byte less, halves the DMA's row run to 128 bytes and doubles
//         the barriers per weight byte - dropped;
//       - v_mfma_f32_32x32x16_bf16 halves the LDS operand READS per product, not the bytes staged, and wants 16 accumulator registers per 32 x 32
//         tile in a layout stream_epilogue's transposed path does not take - dropped.  What is kept for the LDS side is the column-half split: a wave
//         reads half the planes once per chunk (12 KB at eight column tiles) and every weight fragment once.
//   * ring: NIMG = as many images as fit 160 KB, at most four (b9w_nimg: three up to four row tiles next to five or six column tiles, two beyond); chunk c lives in
//     image c % NIMG.  Loader: wait until ITS DMAs of chunk c have landed (vmcnt <= NIW (NIMG - 2)), barrier c, request chunk c + NIMG - 1 into the
//     image chunk c - 1 has left.  MFMA waves: barrier c (behind lgkmcnt(0): their reads of chunk c - 1 are complete), then chunk c out of its image.
//     Image layout and swizzles: stream_b9w_layout.h (k_stream_b9's, through functions both sides call).
// Values: the contract of kernels_gemm_b9.h - exact products for finite inputs of magnitude >= 2^-100 (or 0), nothing promised beyond.
#pragma once
#include "kernels_stream_b9.h"
#include "stream_b9w_layout.h"

namespace lh {

template <int MAXT, int NCT, int NIMG, int NPROD = 8>
__global__ __launch_bounds__(B9S_TH) void k_stream_b9w(const StreamArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.r[2], a.epi, a.gamma, a.ys_plane, a.ldys);   // the argument block's lines behind one wait (kernels_common.h)
    constexpr int KC = B9S_KC;
    static_assert(b9w_built(MAXT, NCT), "row tiles x column tiles");
    static_assert(NIMG >= 2 && NIMG <= 4 && (uint32_t)NIMG * b9w_image_bytes(MAXT, NCT) <= B9W_LDS_BYTES, "ring");
    static_assert(NPROD == 9 || NPROD == 8, "products");
    constexpr int NCW = (int)b9w_ncw(NCT), NCE = 2 * NCW;   // column tiles of an MFMA wave; of the epilogue (even)
    constexpr int NWI = 4 * MAXT, NI = (int)b9w_pieces(MAXT, NCT);
    constexpr int NIW = (NI + 3) / 4;           // DMA instructions per loader wave and chunk
    constexpr int WAITN = NIW * (NIMG - 2) < 64 ? NIW * (NIMG - 2) : 63;
    constexpr uint32_t W_BYTES = b9w_w_bytes(MAXT), XP_BYTES = b9w_plane_bytes(NCT), IMG_BYTES = b9w_image_bytes(MAXT, NCT);
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
        // ---- loader waves: piece q = 4 j + wave of a chunk (stream_b9w_layout.h).  A piece's lanes sit in ONE 16-row tile / one plane, so its first
        // row is a uniform resource base and the lane keeps (row) * pitch + the source granule of the position it lands on
        uint32_t voff[NIW], doff[NIW], sstep[NIW];
        const char* base[NIW];
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            uint32_t q = (uint32_t)j * 4 + (uint32_t)wave;
            q = q < (uint32_t)NI ? q : (uint32_t)NI - 1;                   // surplus slots repeat the last piece (same bytes to the same place)
            const B9wPiece p0 = b9w_piece(MAXT, NCT, q, 0), pl = b9w_piece(MAXT, NCT, q, (uint32_t)lane);   // uniform part; this lane's row and granule
            doff[j] = p0.dst;
            if (q < (uint32_t)NWI) {
                uint32_t ts = p0.row >> 4;                                 // tile slot of the piece: uniform
                ts = ts < nt ? ts : nt - 1;                                // slots beyond the block: a valid tile again, its sums are never stored
                const uint32_t v = t0 + ts;
                uint32_t g, tile;
                if (pairs) { g = v & 1u; tile = v >> 1; }
                else { g = (v >= tiles_per_mat ? 1u : 0u) + (v >= 2 * tiles_per_mat ? 1u : 0u); tile = v - g * tiles_per_mat; }   // (<= 3 matrices: no division)
                base[j] = (const char*)((g == 0 ? a.w[0] : (g == 1 ? a.w[1] : a.w[2])) + (size_t)tile * 16 * a.K + kbase);
                voff[j] = ((pl.row & 15u) * a.K + pl.gran * 4u) * 4u;
                sstep[j] = KC * 4;
            } else {
                const uint32_t c = pl.row < a.n ? pl.row : a.n - 1;        // rows past the batch: the last row again (never stored)
                base[j] = (const char*)(a.xs + (size_t)(p0.kind - 1u) * a.xs_plane + kbase);
                voff[j] = (c * a.ldxs + pl.gran * 8u) * 2u;
                sstep[j] = KC * 2;
            }
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
        wait_vm<0>();                           // the clamped tail requests
    } else {
        // ---- MFMA waves: wave 4 + 2 kb + half
        const uint32_t cw = (uint32_t)(wave - 4), kb = cw >> 1, half = cw & 1u;
#pragma unroll
        for (int j = 0; j < MAXT; ++j)
#pragma unroll
            for (int c = 0; c < NCW; ++c) acc[j][c] = f4m{0.f, 0.f, 0.f, 0.f};
        const uint32_t woff = b9w_w_read_off(0, r16, kb, slot, 0);         // tile slot j: + 4096 j; the fragment's second granule at position ^ 1
        uint32_t xoff[NCW];
#pragma unroll
        for (int c = 0; c < NCW; ++c) xoff[c] = b9w_x_read_off(MAXT, NCT, 0, b9w_col_tile(NCT, half, (uint32_t)c), r16, kb, slot);   // plane p: + p XP_BYTES
        u4 xc[NCW][3];                          // this chunk's operands of the wave's column tiles
        u4 wa[3], wb[3];                        // two weight fragments as three bf16 pieces each, swapped by name
        float raw[8];                           // a fragment as it comes out of LDS
        uint32_t s1[8], s2[8];                  // its residuals on their way into the pieces
        constexpr int P0 = NPROD == 9 ? 0 : 1;
        constexpr int NMT = (9 - P0) * NCW;     // MFMAs per tile
        constexpr int S0 = NMT >= 30 ? 10 : 6;  // first split slot of a tile (the fragment's way from LDS)
        constexpr int NPC = 20;                 // pieces per fragment: 8 splits + 12 permutes
        auto read_w = [&](const char* im, int j, int h) {
            const f4 v = *(const f4*)(im + ((woff + (uint32_t)j * 4096u) ^ (h ? 16u : 0u)));
            raw[4 * h] = v.x; raw[4 * h + 1] = v.y; raw[4 * h + 2] = v.z; raw[4 * h + 3] = v.w;
        };
        auto split_f = [&](int f) {             // 4 vector instructions
            const uint32_t hb = __builtin_bit_cast(uint32_t, raw[f]) & 0xffff0000u;
            const float r1 = __fsub_rn(raw[f], __builtin_bit_cast(float, hb));
            const uint32_t mb = __builtin_bit_cast(uint32_t, r1) & 0xffff0000u;
            s1[f] = __builtin_bit_cast(uint32_t, r1); s2[f] = __builtin_bit_cast(uint32_t, __fsub_rn(r1, __builtin_bit_cast(float, mb)));
            asm volatile("" : "+v"(s1[f]), "+v"(s2[f]));   // (keeps the arithmetic in its slot: kernels_stream_b9.h)
        };
        auto pack1 = [&](u4 (&w)[3], int k) {   // one byte-permute: dword k & 3 of piece k >> 2
            const int pl = k >> 2, d = k & 3;
            const uint32_t lo = pl == 0 ? __builtin_bit_cast(uint32_t, raw[2 * d]) : (pl == 1 ? s1[2 * d] : s2[2 * d]);
            const uint32_t hi = pl == 0 ? __builtin_bit_cast(uint32_t, raw[2 * d + 1]) : (pl == 1 ? s1[2 * d + 1] : s2[2 * d + 1]);
            w[pl][d] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
            asm volatile("" : "+v"(w[pl]));
        };
        // tile j's MFMAs out of `wc`, tile j + 1's fragment on its way into `wn`: reads in slots 0 and 1, the twenty pieces from slot S0 on
        auto tile = [&](const char* im, int j, const u4 (&wc)[3], u4 (&wn)[3]) {
            constexpr int PX[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0}, PW[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0};
#pragma unroll
            for (int m = 0; m < NMT; ++m) {
                const int q = P0 + m / NCW, c = m % NCW;
                acc[j][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xc[c][PX[q]]), __builtin_bit_cast(bf16x8, wc[PW[q]]), acc[j][c], 0, 0, 0);
                if (j + 1 < MAXT) {
                    if (m < 2) read_w(im, j + 1, m);
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
            read_w(im, 0, 0); read_w(im, 0, 1);
#pragma unroll
            for (int c = 0; c < NCW; ++c)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) xc[c][pl] = *(const u4*)(im + xoff[c] + (size_t)pl * XP_BYTES);
#pragma unroll
            for (int f = 0; f < 8; ++f) split_f(f);
#pragma unroll
            for (int k = 0; k < 12; ++k) pack1(wa, k);
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
