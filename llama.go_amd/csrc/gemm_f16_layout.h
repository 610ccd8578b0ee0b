// csrc/gemm_f16_layout.h — the two pure pieces of k_gemm_b9_h (kernels_gemm_f16.h): how a half becomes its bf16 parts, and where the bytes of a ring stage
// sit.  No HIP: the kernel calls these functions, abi.hip exports them (lh_gemm_f16_split / lh_gemm_f16_piece / lh_gemm_f16_w_read_off) and
// tests/test_f16_tiles_cpu.py + tests/gemm_f16_split_main.cpp check them without a GPU.
//
// The split.  split3 (kernels_common.h) of an fp32 w: hi = the top 16 bits of w, r1 = w - hi, mid = the top 16 bits of r1, lo = the top 16 bits of r1 - mid.
// A widened half has at most 11 significant bits: hi keeps 8 of them, r1 holds the other (at most) 3 exactly, so r1's low 16 bits are zero, mid = r1 and
// lo = +0 - for every finite half, subnormal ones included (the smallest non-zero part is 2^-24, far inside split_exact_values' range).  The lo plane is
// therefore never built: two parts per weight.
//
// The stage.  [3 planes][128 rows][32 bf16] of X (k_gemm_b9's slab, 24 KB) | [256 rows][32 halves] of W (16 KB): 40 KB, 64-byte rows everywhere.  A DMA
// piece is 1 KB = 16 rows x four 16-byte granules, lane i at piece base + 16 i, i.e. position i & 3 of row i >> 2; granule g of row r is STORED at position
// g ^ ((r >> 2) & 3), so the lane fetches source granule (i & 3) ^ ((row >> 2) & 3).  40 pieces: 0..23 X (plane p / 8, rows 16 (p % 8) ..), 24..39 W
// (rows 16 (p - 24) ..).  Eight waves take five each (wave w: pieces w, w + 8, .. w + 32): no surplus slot.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_GEMM_H_FN __host__ __device__ inline
#else
#define LH_GEMM_H_FN inline
#endif

namespace lh {

constexpr uint32_t GH_BN = 128, GH_BM = 256, GH_XP_BYTES = GH_BN * 64, GH_W_OFF = 3 * GH_XP_BYTES, GH_STAGE = GH_W_OFF + GH_BM * 64;
constexpr uint32_t GH_XPIECES = 3 * GH_BN / 16, GH_WPIECES = GH_BM / 16, GH_PIECES = GH_XPIECES + GH_WPIECES;

// the fp32 bits of half h: exact, subnormal halves become normal floats (what v_cvt_f32_f16 gives with f16 denormals kept)
LH_GEMM_H_FN uint32_t gemm_h_widen_bits(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, (float)__builtin_bit_cast(_Float16, h));
#else
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, f = h & 0x3ffu;
    if (e == 31) return s | 0x7f800000u | (f << 13);
    if (e) return s | ((e + 112u) << 23) | (f << 13);
    if (!f) return s;
    uint32_t sh = 0, m = f;
    while (!(m & 0x400u)) { m <<= 1; ++sh; }          // normalise: value = f * 2^-24
    return s | ((113u - sh) << 23) | ((m & 0x3ffu) << 13);
#endif
}
// the weight split of k_gemm_b9_h: *w = the widened half (its top 16 bits are the hi part), *r1 = w - hi (its top 16 bits are the mid part, its low 16
// bits zero for every finite half)
LH_GEMM_H_FN void gemm_h_split(uint16_t h, uint32_t* w, uint32_t* r1) {
    const uint32_t wb = gemm_h_widen_bits(h), hb = wb & 0xffff0000u;
    float wf, hf;
#if defined(__HIP_DEVICE_COMPILE__)
    wf = __builtin_bit_cast(float, wb); hf = __builtin_bit_cast(float, hb);
    const float r = __fsub_rn(wf, hf);
    *w = wb; *r1 = __builtin_bit_cast(uint32_t, r);
#else
    memcpy(&wf, &wb, 4); memcpy(&hf, &hb, 4);
    const float r = wf - hf;
    *w = wb; memcpy(r1, &r, 4);
#endif
}

// granule g (0..3) of a 64-byte row r is stored at this position of the row (an involution in g)
LH_GEMM_H_FN uint32_t gemm_h_granule_pos(uint32_t r, uint32_t g) { return g ^ ((r >> 2) & 3u); }
// DMA piece p (0..39), lane (0..63): byte offset in the stage the lane's 16 bytes land at
LH_GEMM_H_FN uint32_t gemm_h_piece_dst(uint32_t p, uint32_t lane) { return p * 1024u + lane * 16u; }
// ... the row the lane fetches from: plane-local X tile row (p < 24; plane = p / 8) or W tile row
LH_GEMM_H_FN uint32_t gemm_h_piece_row(uint32_t p, uint32_t lane) { return (p < GH_XPIECES ? (p % (GH_BN / 16)) : (p - GH_XPIECES)) * 16u + (lane >> 2); }
// ... and the source granule of that row's slab columns (granule g = columns 8 g .. 8 g + 7)
LH_GEMM_H_FN uint32_t gemm_h_piece_granule(uint32_t p, uint32_t lane) { return gemm_h_granule_pos(gemm_h_piece_row(p, lane), lane & 3u); }
// byte offset in the stage of the 16 bytes (8 halves: slab columns 16 kk + 8 lh ..) lane (li = weight row in the 32-row tile, lh) of the wave holding tile
// rows 32 wm .. reads for k-step kk
LH_GEMM_H_FN uint32_t gemm_h_w_read_off(uint32_t wm, uint32_t li, uint32_t lh, uint32_t kk) {
    const uint32_t r = wm * 32u + li;
    return GH_W_OFF + r * 64u + gemm_h_granule_pos(r, 2u * kk + lh) * 16u;
}

}  // namespace lh
