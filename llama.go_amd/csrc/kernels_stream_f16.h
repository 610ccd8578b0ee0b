// csrc/kernels_stream_f16.h — the weight-streaming MFMA kernels of 2..128 token rows over f16 weight matrices kept f16 in HBM (dtype 1).
//
// k_stream_mm2_h / k_stream_dma_h are k_stream_mm2 / k_stream_dma (kernels_stream.h) with ONE difference: how a weight gets from HBM to the MFMA
// operand register.  Widening a half is exact, and everything the sums depend on is the fp32 kernels': the k-deal (KC, KA, CS, the k-blocks of a wave,
// ksplit), the MFMA sequence per wave, the wave order in stream_epilogue (shared, not restated).  So a launch computes the bits of the fp32 kernel of the
// same template arguments over the widened matrix.  StreamArgs is the fp32 kernels': w[] points at halves, [M][K] row-major, 2 K bytes per row.
//   * k_stream_mm2_h: the loader waves fetch four HALVES per lane and register on the fp32 lane map (8-byte non-temporal loads), widen them in
//     registers (v_cvt_f32_f16, f16 denormals kept - widen4, kernels_f16.h) and write the fp32 image the fp32 loader writes, with the same
//     ds_write_b128s.  The activation / gamma staging, the folded norm's sums, the MFMA waves and the operand pipeline are k_stream_mm2's text.
//   * k_stream_dma_h: the weight part of every ring image holds halves.  An LDS-DMA instruction still moves 16 bytes per lane = 8 halves, so 1 KB covers
//     8 weight rows at KC = 64 (128-byte rows) and 4 at KC = 128: inside one 16-row tile, the uniform resource base survives.  The activation rows stay
//     fp32 in k_stream_dma's layout.  An MFMA lane reads its 4 halves of a k-block with one ds_read_b64, widens them and issues k_stream_dma's MFMAs.
// Clamps (rows past nt * 16, columns past n, chunks past nch) are the fp32 kernels' and every clamped address stays inside the halved extent:
// a clamped tile slot is a tile of the block, its rows tile * 16 + (0..15) < M; a chunk index <= nch - 1 with (ch0 + nch) KC <= K; a lane's column
// offset < KC - so the last byte read of a row is at most 2 K - 1 of that row ("Native stream kernels").
#pragma once
#include "kernels_f16.h"
#include "kernels_stream.h"
#include "stream_f16_layout.h"

namespace lh {

// (the weight image of k_stream_dma_h: stream_f16_layout.h)
__host__ __device__ constexpr size_t stream_dma_h_image_bytes(int maxt, int nct, int kc) { return (size_t)maxt * 16 * kc * 2 + (size_t)nct * 16 * kc * 4; }

// ---------------------------------------------------------------------------------------------------------------------------------
// chunks in flight in the loader waves' registers: k_stream_mm2's choice per shape (a set of halves is half the registers AND half the bytes;
// more sets are unmeasured).  -DSTREAM_H_NS=n overrides for probe builds.
#ifndef STREAM_H_NS
#define STREAM_H_NS 2
#endif
template <int MAXT, int NCT, int KC>
__global__ __launch_bounds__(2 * ST_TH) void k_stream_mm2_h(const StreamArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.r[2], a.epi, a.gamma, a.ys_plane, a.ldys);
    static_assert(KC == 64 || KC == 128 || KC == 256, "chunk");
    constexpr int ST_PITCH = KC + 4, RPP = 1024 / KC;
    constexpr int NW = MAXT * 16 / RPP, NX = NCT * 16 / RPP;
    constexpr size_t IMG = (size_t)(MAXT + NCT) * 16 * ST_PITCH;      // floats per image: the fp32 kernel's image
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* img = (float*)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles_per_mat = a.M >> 4, T = tiles_per_mat * a.groups;
    const bool pairs = a.epi == ST_EPI_SILU_MUL;
    const uint32_t units = pairs ? tiles_per_mat : T, um = pairs ? 2u : 1u;
    const uint32_t S = a.ksplit > 1 ? a.ksplit : 1u, bg = (uint32_t)blockIdx.x / S, ks = (uint32_t)blockIdx.x - bg * S, ng = (uint32_t)gridDim.x / S;
    if (bg >= ng) return;
    const uint32_t t0 = um * (uint32_t)(((uint64_t)bg * units) / ng), t1 = um * (uint32_t)(((uint64_t)(bg + 1) * units) / ng);
    if (t1 <= t0) return;
    auto tile_of = [&](uint32_t v, uint32_t* g, uint32_t* tile) {
        if (pairs) { *g = v & 1u; *tile = v >> 1; }
        else { *g = (v >= tiles_per_mat ? 1u : 0u) + (v >= 2 * tiles_per_mat ? 1u : 0u); *tile = v - *g * tiles_per_mat; }
    };
    const uint32_t nt = t1 - t0;
    const uint32_t nch_all = a.K / KC, ch0 = (uint32_t)(((uint64_t)ks * nch_all) / S);
    const uint32_t nch = (uint32_t)(((uint64_t)(ks + 1) * nch_all) / S) - ch0;
    const uint32_t kbase = ch0 * KC;
    if (nch == 0) return;
    typedef const f4 __attribute__((address_space(1))) gf4;
    typedef const h4 __attribute__((address_space(1))) gh4;
    constexpr int KB = KC / 64;
    constexpr int KA0 = (MAXT * NCT >= 4) ? 1 : (MAXT * NCT >= 2 ? 2 : 4), KA = KA0 < KB ? KA0 : KB;
    constexpr bool PIPE = STREAM_PIPE != 0 && KC == 64 && NCT >= 2 && NCT <= 5;
    f4m acc[KA][MAXT][NCT];
    const uint32_t r16 = (uint32_t)lane & 15, slot = (uint32_t)lane >> 4;
    if (wave < 4) {
        // ---- loader waves: k_stream_mm2's, the weights as halves
        const uint32_t rsub = (uint32_t)tid / (KC / 4), seg = (uint32_t)tid % (KC / 4);
        const float* xp[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            uint32_t c = (uint32_t)i * RPP + rsub;
            c = c < a.n ? c : a.n - 1;
            xp[i] = a.x + (size_t)c * a.ldx + kbase + seg * 4;
        }
        constexpr int NS = (STREAM_H_NS == 2 && MAXT == 1 && NCT == 1) ? 4 : STREAM_H_NS;
        const float* gp = (a.gamma ? a.gamma : a.x) + kbase + seg * 4;
        const bool norm = a.gamma != nullptr;
        double ssq[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) ssq[i] = 0.0;
        auto stash_x = [&](const f4 (&xr)[NX], const f4& gq, float* im) {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                f4 v = xr[i];
                if (norm) {
                    ssq[i] += (double)__fadd_rn(__fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)), __fadd_rn(__fmul_rn(v.z, v.z), __fmul_rn(v.w, v.w)));
                    v.x = __fmul_rn(gq.x, v.x); v.y = __fmul_rn(gq.y, v.y); v.z = __fmul_rn(gq.z, v.z); v.w = __fmul_rn(gq.w, v.w);
                }
                *(f4*)(im + (size_t)(MAXT * 16 + i * RPP + rsub) * ST_PITCH + seg * 4) = v;
            }
        };
        auto publish_scales = [&]() {
            if (!norm) return;
            float* scl = img + 2 * IMG;
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                double t = ssq[i];
#pragma unroll
                for (int o = KC / 8; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
                if (seg == 0) scl[i * RPP + rsub] = (float)(1.0 / sqrt(t / (double)a.K + 1e-5));
            }
        };
        {
        const _Float16* wp[NW];      // the lane's four halves of register i's row: element offsets as in the fp32 kernel, two bytes each
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            uint32_t rr = (uint32_t)i * RPP + rsub;
            rr = rr < nt * 16 ? rr : nt * 16 - 1;
            uint32_t g, tile;
            tile_of(t0 + (rr >> 4), &g, &tile);
            const uint32_t row = tile * 16 + (rr & 15);
            const uint64_t base = (uint64_t)a.w[0] + (g >= 1 ? (uint64_t)a.w[1] - (uint64_t)a.w[0] : 0) + (g == 2 ? (uint64_t)a.w[2] - (uint64_t)a.w[1] : 0);
            wp[i] = (const _Float16*)base + (size_t)row * a.K + kbase + seg * 4;
        }
        constexpr bool BUF = NCT >= 2;
        __amdgpu_buffer_rsrc_t wres[NW], xres = stream_rsrc(a.x + kbase), gres = stream_rsrc((a.gamma ? a.gamma : a.x) + kbase);
        uint32_t wvo[NW], xvo[NX];
        if constexpr (BUF) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const uint32_t ts0 = ((uint32_t)i * RPP) >> 4, ts = ts0 < nt ? ts0 : nt - 1;
                uint32_t g, tile;
                tile_of(t0 + ts, &g, &tile);
                const _Float16* mb = (const _Float16*)(g == 0 ? a.w[0] : (g == 1 ? a.w[1] : a.w[2]));
                wres[i] = stream_rsrc(mb + (size_t)tile * 16 * a.K + kbase);
                uint32_t rr = (uint32_t)i * RPP + rsub;
                rr = rr < nt * 16 ? rr : nt * 16 - 1;
                wvo[i] = ((rr & 15u) * a.K + seg * 4u) * 2u;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                uint32_t c = (uint32_t)i * RPP + rsub;
                c = c < a.n ? c : a.n - 1;
                xvo[i] = (c * a.ldx + seg * 4u) * 4u;
            }
        }
        h4 ws[NS][NW];
        f4 xs[NS][NX], gs[NS];
        auto issue = [&](h4 (&wr)[NW], f4 (&xr)[NX], f4& gq, uint32_t ch) {
            const uint32_t k0 = (ch < nch ? ch : nch - 1) * KC;
            if constexpr (BUF) {
#pragma unroll
                for (int i = 0; i < NW; ++i) wr[i] = __builtin_bit_cast(h4, __builtin_amdgcn_raw_buffer_load_b64(wres[i], wvo[i], k0 * 2u, 2 /* nt */));
                const uint32_t so = k0 * 4u;
#pragma unroll
                for (int i = 0; i < NX; ++i) xr[i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(xres, xvo[i], so, 0));
                gq = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(gres, seg * 16u, so, 0));
                return;
            }
#pragma unroll
            for (int i = 0; i < NW; ++i) wr[i] = __builtin_nontemporal_load((gh4*)(uintptr_t)(wp[i] + k0));
#pragma unroll
            for (int i = 0; i < NX; ++i) xr[i] = *(gf4*)(uintptr_t)(xp[i] + k0);
            gq = *(gf4*)(uintptr_t)(gp + k0);
        };
        auto stash = [&](const h4 (&wr)[NW], const f4 (&xr)[NX], const f4& gq, float* im) {
#pragma unroll
            for (int i = 0; i < NW; ++i) *(f4*)(im + (size_t)(i * RPP + rsub) * ST_PITCH + seg * 4) = widen4(wr[i]);   // the fp32 image
            stash_x(xr, gq, im);
        };
        constexpr int PER_SET = NW + NX + 1;
        static_assert(PER_SET * (NS - 1) < 64 || STREAM_H_NS != 2, "vmcnt range");
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            issue(ws[q], xs[q], gs[q], (uint32_t)q);
            __builtin_amdgcn_sched_barrier(0);
        }
        uint32_t ch = 0;
        for (; ch + NS <= nch; ch += NS) {
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                wait_vm<(PER_SET * (NS - 1) < 64 ? PER_SET * (NS - 1) : 63)>();
                stash(ws[q], xs[q], gs[q], ((ch + q) & 1) ? img + IMG : img);
                issue(ws[q], xs[q], gs[q], ch + q + NS);
                __syncthreads();
            }
        }
        const uint32_t rem = nch - ch;
#pragma unroll
        for (int q = 0; q < NS - 1; ++q) {
            if ((uint32_t)q < rem) {
                if (q == 0) wait_vm<(PER_SET * (NS - 1) < 64 ? PER_SET * (NS - 1) : 63)>();
                else if (q == 1) wait_vm<(PER_SET * (NS > 2 ? NS - 2 : 0) < 64 ? PER_SET * (NS > 2 ? NS - 2 : 0) : 63)>();
                else wait_vm<(PER_SET * (NS > 3 ? NS - 3 : 0) < 64 ? PER_SET * (NS > 3 ? NS - 3 : 0) : 63)>();
                stash(ws[q], xs[q], gs[q], ((ch + q) & 1) ? img + IMG : img);
                __syncthreads();
            }
        }
        wait_vm<0>();
        publish_scales();
        }
        if constexpr (PIPE) { __syncthreads(); __syncthreads(); }
    } else {
        // ---- compute waves: k_stream_mm2's (the image is the fp32 kernel's)
        const int cw = wave - 4;
#pragma unroll
        for (int q = 0; q < KA; ++q)
#pragma unroll
            for (int t = 0; t < MAXT; ++t)
#pragma unroll
                for (int c = 0; c < NCT; ++c) acc[q][t][c] = f4m{0.f, 0.f, 0.f, 0.f};
        auto compute = [&](const float* im) {
            const float* Wt = im;
            const float* Xt = im + (size_t)MAXT * 16 * ST_PITCH;
            constexpr int HB = KB >= 2 ? 2 : 1;
#pragma unroll
            for (int h0 = 0; h0 < KB; h0 += HB) {
                f4 bf[HB][NCT], af[HB][MAXT];
#pragma unroll
                for (int hh = 0; hh < HB; ++hh) {
                    const uint32_t koff = (uint32_t)(KB * cw + h0 + hh) * 16 + slot * 4;
#pragma unroll
                    for (int c = 0; c < NCT; ++c) bf[hh][c] = *(const f4*)(Xt + (size_t)(c * 16 + r16) * ST_PITCH + koff);
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) af[hh][t] = *(const f4*)(Wt + (size_t)(t * 16 + r16) * ST_PITCH + koff);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int hh = 0; hh < HB; ++hh)
#pragma unroll
                        for (int t = 0; t < MAXT; ++t)
#pragma unroll
                            for (int c = 0; c < NCT; ++c)
                                acc[(h0 + hh) % KA][t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[hh][t][s], bf[hh][c][s], acc[(h0 + hh) % KA][t][c], 0, 0, 0);
            }
        };
        if constexpr (PIPE) {
            constexpr int NO = MAXT + NCT;
            f4 ops[2][KB][NO];
            auto read_ops = [&](f4 (&o)[KB][NO], const float* im) {
                const float* Wt = im;
                const float* Xt = im + (size_t)MAXT * 16 * ST_PITCH;
#pragma unroll
                for (int h = 0; h < KB; ++h) {
                    const uint32_t koff = (uint32_t)(KB * cw + h) * 16 + slot * 4;
#pragma unroll
                    for (int c = 0; c < NCT; ++c) o[h][MAXT + c] = *(const f4*)(Xt + (size_t)(c * 16 + r16) * ST_PITCH + koff);
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) o[h][t] = *(const f4*)(Wt + (size_t)(t * 16 + r16) * ST_PITCH + koff);
                }
            };
            auto mfmas = [&](const f4 (&o)[KB][NO]) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int h = 0; h < KB; ++h)
#pragma unroll
                        for (int t = 0; t < MAXT; ++t)
#pragma unroll
                            for (int c = 0; c < NCT; ++c)
                                acc[h % KA][t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(o[h][t][s], o[h][MAXT + c][s], acc[h % KA][t][c], 0, 0, 0);
            };
            __syncthreads();
            read_ops(ops[0], img);
            __syncthreads();
            for (uint32_t ch = 0; ch < nch; ch += 2) {
                if (ch + 1 < nch) read_ops(ops[1], img + IMG);
                __builtin_amdgcn_sched_barrier(0);
                mfmas(ops[0]);
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
                if (ch + 1 < nch) {
                    if (ch + 2 < nch) read_ops(ops[0], img);
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(ops[1]);
                    __builtin_amdgcn_sched_barrier(0);
                    __syncthreads();
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
            for (uint32_t ch = 0; ch < nch; ++ch) {
                __syncthreads();
                compute((ch & 1) ? img + IMG : img);
            }
        }
    }
    __syncthreads();
    stream_epilogue<MAXT, NCT>(a, smem_raw, (uint32_t)(2 * IMG), a.gamma ? (const float*)smem_raw + 2 * IMG : nullptr, t0, nt, ks, tiles_per_mat, [&](int t, int c) {
        f4m v = acc[0][t][c];
#pragma unroll
        for (int q = 1; q < KA; ++q) v += acc[q][t][c];
        return v;
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k_stream_dma_h: ring image = [MAXT * 16 weight rows][KC halves] (stream_h_granule_off), then [NCT * 16 activation rows][KC floats] (k_stream_dma's
// part: granule g of row r at g ^ (r & 15)).  Pieces of 1 KB: RPW weight rows (8 | 4) or RPX activation rows (4 | 2) each; piece q = 4 j + wave is
// instruction j of loader wave `wave`, the weight pieces first.  The piece count is not a multiple of four (MAXT = 1, KC = 64: 2 weight pieces), so
// every wave issues NIW = ceil(pieces / 4) instructions and a surplus slot repeats the last piece - the same bytes to the same place - as k_stream_b9
// deals its mixed pieces: the counted vmcnt wait is then one constant.
template <int MAXT, int NCT, int KC, int NIMG, bool PIPE, int CS = 1>
__global__ __launch_bounds__(2 * ST_TH) void k_stream_dma_h(const StreamArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.r[2], a.epi, a.gamma, a.ys_plane, a.ldys);
    static_assert(KC == 64 || KC == 128, "chunk");
    static_assert(NIMG >= 2 && NIMG <= 5, "ring");
    constexpr int GRW = KC / 8, RPW = 64 / GRW;     // 16-byte granules per weight row of halves; weight rows per DMA instruction
    constexpr int GRX = KC / 4, RPX = 64 / GRX;     // the same for the fp32 activation rows
    constexpr int NWI = MAXT * 16 / RPW, NXI = NCT * 16 / RPX, NI = NWI + NXI;
    constexpr int NIW = (NI + 3) / 4;               // DMA instructions per loader wave and chunk
    constexpr int WAITN = NIW * (NIMG - 2) < 64 ? NIW * (NIMG - 2) : 63;
    constexpr uint32_t W_BYTES = MAXT * 16 * KC * 2, IMG_BYTES = W_BYTES + NCT * 16 * KC * 4;
    static_assert(16 % RPW == 0 && 16 % RPX == 0, "a piece sits in one tile");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles_per_mat = a.M >> 4, T = tiles_per_mat * a.groups;
    const bool pairs = a.epi == ST_EPI_SILU_MUL;
    const uint32_t units = pairs ? tiles_per_mat : T, um = pairs ? 2u : 1u;
    const uint32_t S = a.ksplit > 1 ? a.ksplit : 1u, bg = (uint32_t)blockIdx.x / S, ks = (uint32_t)blockIdx.x - bg * S, ng = (uint32_t)gridDim.x / S;
    if (bg >= ng) return;
    const uint32_t t0 = um * (uint32_t)(((uint64_t)bg * units) / ng), t1 = um * (uint32_t)(((uint64_t)(bg + 1) * units) / ng);
    if (t1 <= t0) return;
    const uint32_t nt = t1 - t0;                // <= MAXT (host)
    const uint32_t nch_all = a.K / KC, ch0 = (uint32_t)(((uint64_t)ks * nch_all) / S);
    const uint32_t nch = (uint32_t)(((uint64_t)(ks + 1) * nch_all) / S) - ch0;
    const uint32_t kbase = ch0 * KC;
    if (nch == 0) return;
    const uint32_t r16 = (uint32_t)lane & 15, slot = (uint32_t)lane >> 4;
    static_assert(CS == 1 || (CS == 2 && NCT % 2 == 0), "column split");
    constexpr int NKG = 4 / CS, NCW = NCT / CS;
    constexpr int KB = KC / 16 / NKG;           // k-blocks (of 16 columns) per MFMA wave and chunk
    f4m acc[MAXT][NCW];
    if (wave < 4) {
        uint32_t voff[NIW], doff[NIW], sstep[NIW];
        const char* base[NIW];
#pragma unroll
        for (int j = 0; j < NIW; ++j) {
            uint32_t q = (uint32_t)j * 4 + (uint32_t)wave;
            q = q < (uint32_t)NI ? q : (uint32_t)NI - 1;                   // surplus slots repeat the last piece
            if (q < (uint32_t)NWI) {
                const uint32_t rr = q * RPW + (uint32_t)lane / GRW;        // image row this lane feeds
                const uint32_t gd = (uint32_t)lane % GRW;                  // granule position it lands on
                const uint32_t gs = stream_h_granule_pos(KC, rr, gd);      // source granule stored there (an involution)
                uint32_t ti = (q * RPW) >> 4;                              // tile slot of the instruction: uniform
                ti = ti < nt ? ti : nt - 1;                                // slots beyond the block: a valid tile again, its sums are never stored
                const uint32_t v = t0 + ti;
                uint32_t g, tile;
                if (pairs) { g = v & 1u; tile = v >> 1; }
                else { g = (v >= tiles_per_mat ? 1u : 0u) + (v >= 2 * tiles_per_mat ? 1u : 0u); tile = v - g * tiles_per_mat; }
                const _Float16* mb = (const _Float16*)(g == 0 ? a.w[0] : (g == 1 ? a.w[1] : a.w[2]));
                base[j] = (const char*)(mb + (size_t)tile * 16 * a.K + kbase);
                voff[j] = ((rr & 15u) * a.K + gs * 8u) * 2u;
                sstep[j] = KC * 2;
                doff[j] = q * 1024u;
            } else {
                const uint32_t xi = q - NWI;
                const uint32_t rr = xi * RPX + (uint32_t)lane / GRX, gd = (uint32_t)lane % GRX, gs = gd ^ (rr & 15u);
                const uint32_t c = rr < a.n ? rr : a.n - 1;                // columns past the batch: the last row again (never stored)
                base[j] = (const char*)(a.x + kbase);
                voff[j] = (c * a.ldx + gs * 4u) * 4u;
                sstep[j] = KC * 4;
                doff[j] = W_BYTES + xi * 1024u;
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
                if (doff[j] < W_BYTES) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, (int)voff[j], so, 0, STREAM_DMA_WAUX);   // weights: read once (nt)
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, (int)voff[j], so, 0, 0);                                   // activations: out of L2
            }
        };
#pragma unroll
        for (int c = 0; c < NIMG - 1; ++c) issue((uint32_t)c);
        for (uint32_t ch = 0; ch < nch; ++ch) {
            wait_vm<WAITN>();
            __builtin_amdgcn_s_barrier();
            issue(ch + NIMG - 1);
        }
        if constexpr (PIPE) __builtin_amdgcn_s_barrier();
        wait_vm<0>();
    } else {
        // ---- MFMA waves: k_stream_dma's, the weight operands as four halves per lane and k-block
        const int cw = wave - 4;
        const uint32_t kq = CS == 2 ? (uint32_t)cw >> 1 : (uint32_t)cw, c0 = CS == 2 ? ((uint32_t)cw & 1u) * NCW : 0u;
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
#pragma unroll
            for (int c = 0; c < NCW; ++c) acc[t][c] = f4m{0.f, 0.f, 0.f, 0.f};
        struct Ops { h4 w[MAXT]; f4 x[NCW]; };
        auto read_kb = [&](Ops& o, const char* im, int h) {   // operands of this wave's k-block h of the chunk in `im`
            const uint32_t kb = kq * KB + (uint32_t)h;
            const uint32_t g = (kb * 4 + slot) ^ r16;
            const float* Xt = (const float*)(im + W_BYTES);
#pragma unroll
            for (int c = 0; c < NCW; ++c) o.x[c] = *(const f4*)(Xt + ((size_t)((c0 + c) * 16 + r16) * GRX + g) * 4);
#pragma unroll
            for (int t = 0; t < MAXT; ++t) o.w[t] = *(const h4*)(im + stream_h_read_off(KC, (uint32_t)t, r16, kb, slot));
        };
        auto mfma_kb = [&](const Ops& o) {
            f4 wf[MAXT];
#pragma unroll
            for (int t = 0; t < MAXT; ++t) wf[t] = widen4(o.w[t]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < MAXT; ++t)
#pragma unroll
                    for (int c = 0; c < NCW; ++c) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t][s], o.x[c][s], acc[t][c], 0, 0, 0);
        };
        auto image = [&](uint32_t ch) { return (const char*)(smem_raw + (size_t)(ch % NIMG) * IMG_BYTES); };
        if constexpr (PIPE) {
            static_assert(KB == 1 || KB == 2, "k-blocks per wave and chunk");
            Ops opa, opb;
            barrier_lds_only();
            read_kb(opa, smem_raw, 0);
            if constexpr (KB == 2) {
                for (uint32_t ch = 0; ch < nch; ++ch) {
                    read_kb(opb, image(ch), 1);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_kb(opa);
                    __builtin_amdgcn_sched_barrier(0);
                    barrier_lds_only();
                    if (ch + 1 < nch) read_kb(opa, image(ch + 1), 0);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_kb(opb);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                for (uint32_t ch = 0; ch < nch; ch += 2) {
                    barrier_lds_only();
                    if (ch + 1 < nch) read_kb(opb, image(ch + 1), 0);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_kb(opa);
                    __builtin_amdgcn_sched_barrier(0);
                    if (ch + 1 < nch) {
                        barrier_lds_only();
                        if (ch + 2 < nch) read_kb(opa, image(ch + 2), 0);
                        __builtin_amdgcn_sched_barrier(0);
                        mfma_kb(opb);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        } else {
            for (uint32_t ch = 0; ch < nch; ++ch) {
                barrier_lds_only();
                Ops ops[KB];
#pragma unroll
                for (int h = 0; h < KB; ++h) read_kb(ops[h], image(ch), h);
#pragma unroll
                for (int h = 0; h < KB; ++h) mfma_kb(ops[h]);
            }
        }
    }
    __syncthreads();   // the images are dead (the loader waves have drained their DMAs)
    stream_epilogue<MAXT, NCT, CS>(a, smem_raw, (uint32_t)((size_t)NIMG * IMG_BYTES / 4), nullptr, t0, nt, ks, tiles_per_mat, [&](int t, int c) { return acc[t][c]; });
}

}  // namespace lh
