// csrc/stream_q41_layout.h — where the bytes of a Q4_1 weight chunk sit in the weight part of a ring image of k_stream_dma_q41 (kernels_stream_q41.h): pure
// functions (no HIP), called by the kernel's loader waves AND by its MFMA waves, exported as lh_stream_q41_* and unit-tested without a GPU
// (tests/test_q41_stream_cpu.py).
//
// A chunk of kc columns (64 | 128) of one weight row is kc / 32 nibble granules (16 bytes = one quant block: byte b holds column 2 b low, 2 b + 1 high) and
// kc / 64 pair granules (16 bytes = (d, m) of blocks 2 c and 2 c + 1, contiguous in the (d, m) plane).  The weight part of an image of maxt tile slots:
//   [maxt * 16 rows][kc / 32 nibble granules]   then   [maxt * 16 rows][kc / 64 pair granules]   then padding up to a multiple of 1 KB
// - 768 bytes per tile at kc = 64, 1536 at 128 (fp32: 4 KB / 8 KB).  It is DENSE and granule-linear: LDS-DMA instruction q writes lane i at 1024 q + 16 i, so
// the loader numbers the granules 0 .. stream_q41_granules - 1 in image order, lane i of instruction q brings granule 64 q + i from wherever it lives in HBM
// (per-lane addresses: an instruction spans tiles, both planes and, for (w1, w3) tile pairs, two matrices), and the lanes past the last granule land in the
// padding.  No row can be padded, so the permutation that keeps the operand reads conflict-free goes on the SOURCE side: granule g of image row r is
// stored at position stream_q41_nib_pos / _pair_pos (an involution in g for a fixed row - loader and reader call the same function).
// Bank model (stream_f16_layout.h: 64 banks of 4 bytes, a read is served per half-wave of 32 lanes; lanes that read the same address share one access).
// A half-wave is 16 rows x slots (s, s + 1) of one k-block; both slots of a row read the same dword / the same 8 bytes, so 16 rows must fall on 16
// different banks (ds_read_b32) / bank pairs (ds_read_b64):
//   nibbles, kc = 64:  32-byte rows, rows r and r + 8 would collide: position b ^ (r >> 3 & 1)  -> bank 8 (r & 7) + 4 pos + dword, 16 different;
//   nibbles, kc = 128: 64-byte rows, rows r, r + 4, r + 8, r + 12 would: position b ^ (r >> 2 & 3) -> bank 16 (r & 3) + 4 pos + dword;
//   pairs, kc = 64:    16-byte rows: bank 4 r + 2 (block & 1), no collision, no swizzle;
//   pairs, kc = 128:   32-byte rows, r and r + 8 would: position c ^ (r >> 3 & 1).
// Tile slots are 512 B / 1 KB (nibbles) and 256 / 512 B (pairs) apart - multiples of the 256-byte bank line - and the pair region starts at one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_STREAM_Q41_FN __host__ __device__ inline constexpr
#else
#define LH_STREAM_Q41_FN inline constexpr
#endif

namespace lh {

LH_STREAM_Q41_FN uint32_t stream_q41_gn(uint32_t kc) { return kc / 32u; }   // nibble granules per image row
LH_STREAM_Q41_FN uint32_t stream_q41_gp(uint32_t kc) { return kc / 64u; }   // pair granules per image row
LH_STREAM_Q41_FN uint32_t stream_q41_nib_granules(uint32_t kc, uint32_t maxt) { return maxt * 16u * stream_q41_gn(kc); }
LH_STREAM_Q41_FN uint32_t stream_q41_granules(uint32_t kc, uint32_t maxt) { return maxt * 16u * (stream_q41_gn(kc) + stream_q41_gp(kc)); }
// bytes of the weight part: whole LDS-DMA instructions
LH_STREAM_Q41_FN uint32_t stream_q41_weight_bytes(uint32_t kc, uint32_t maxt) { return (stream_q41_granules(kc, maxt) * 16u + 1023u) & ~1023u; }
LH_STREAM_Q41_FN uint32_t stream_q41_nib_pos(uint32_t kc, uint32_t r, uint32_t g) { return kc == 64 ? g ^ ((r >> 3) & 1u) : g ^ ((r >> 2) & 3u); }
LH_STREAM_Q41_FN uint32_t stream_q41_pair_pos(uint32_t kc, uint32_t r, uint32_t g) { return kc == 64 ? g : g ^ ((r >> 3) & 1u); }
// byte offset, in the weight part, of nibble granule g (plane 0: quant block g of the chunk) / pair granule g (plane 1: blocks 2 g, 2 g + 1) of image row r
LH_STREAM_Q41_FN uint32_t stream_q41_granule_off(uint32_t kc, uint32_t maxt, uint32_t plane, uint32_t r, uint32_t g) {
    return plane == 0 ? (r * stream_q41_gn(kc) + stream_q41_nib_pos(kc, r, g)) * 16u
                      : (stream_q41_nib_granules(kc, maxt) + r * stream_q41_gp(kc) + stream_q41_pair_pos(kc, r, g)) * 16u;
}
// the loader's side: what lands at granule position L (< stream_q41_granules) of the weight part
struct StreamQ41Granule { uint32_t plane, row, g; };
LH_STREAM_Q41_FN StreamQ41Granule stream_q41_granule_src(uint32_t kc, uint32_t maxt, uint32_t L) {
    const uint32_t nn = stream_q41_nib_granules(kc, maxt);
    if (L < nn) { const uint32_t r = L / stream_q41_gn(kc); return {0u, r, stream_q41_nib_pos(kc, r, L % stream_q41_gn(kc))}; }
    const uint32_t r = (L - nn) / stream_q41_gp(kc);
    return {1u, r, stream_q41_pair_pos(kc, r, (L - nn) % stream_q41_gp(kc))};
}
// the reader's side, MFMA lane (r16, slot) of tile slot t, k-block kb (< kc / 16) of the chunk: columns 16 kb + 4 slot .. + 3 of the row are the two bytes
// at stream_q41_read_off - half (slot & 1) of the aligned dword the lane reads - and their block's (d, m) the 8 bytes at stream_q41_pair_off
LH_STREAM_Q41_FN uint32_t stream_q41_read_off(uint32_t kc, uint32_t maxt, uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot) {
    return stream_q41_granule_off(kc, maxt, 0u, t * 16u + r16, kb >> 1) + (kb & 1u) * 8u + slot * 2u;
}
LH_STREAM_Q41_FN uint32_t stream_q41_pair_off(uint32_t kc, uint32_t maxt, uint32_t t, uint32_t r16, uint32_t kb) {
    return stream_q41_granule_off(kc, maxt, 1u, t * 16u + r16, kb >> 2) + ((kb >> 1) & 1u) * 8u;
}

}  // namespace lh
