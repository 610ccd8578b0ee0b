// csrc/stream_f16_layout.h — where a half sits in the weight part of a ring image of k_stream_dma_h (kernels_stream_f16.h): pure functions (no HIP),
// called by the kernel's loader waves AND by its MFMA waves, exported as lh_stream_f16_image_off / lh_stream_f16_read_off and unit-tested without a GPU
// (tests/test_f16_stream_cpu.py, tests/stream_f16_layout_main.cpp).
//
// Image row r (weight row r & 15 of tile slot r >> 4) holds the kc halves of the chunk as kc / 8 granules of 16 bytes (granule g = columns 8 g .. 8 g + 7 of
// the chunk), row pitch 2 kc bytes, dense: an LDS-DMA instruction writes lane i at base + 16 i, so no row can be padded and the permutation that keeps the
// operand reads conflict-free goes on the SOURCE address.  Granule g of row r is stored at position stream_h_granule_pos(kc, r, g): an involution in g
// for a fixed row, so the loader (which picks the source granule for the position its lane lands on) and the reader call the same function.
// Under the LDS bank model (ds_read_b64: two 32-lane halves, bank (address / 4) % 64) the 32 lanes of a half - 16 rows x slots s, s + 1 of one k-block,
// which share ONE granule index - touch 32 different 8-byte units:
//   128-byte rows (kc = 64): two rows per bank line; rows 2 p and 2 p + 1 share the swizzle p (the one k_stream_b9 uses for its planes);
//   256-byte rows (kc = 128): every row starts at bank 0; sixteen swizzles.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_STREAM_H_FN __host__ __device__ inline
#else
#define LH_STREAM_H_FN inline
#endif

namespace lh {

LH_STREAM_H_FN uint32_t stream_h_granule_pos(uint32_t kc, uint32_t r, uint32_t g) { return kc == 64 ? g ^ ((r >> 1) & 7u) : g ^ (r & 15u); }
// byte offset, in the weight part of an image, of granule g of image row r
LH_STREAM_H_FN uint32_t stream_h_granule_off(uint32_t kc, uint32_t r, uint32_t g) { return r * kc * 2u + stream_h_granule_pos(kc, r, g) * 16u; }
// byte offset of the 8 bytes MFMA lane (r16, slot) reads of tile slot t for k-block kb of the chunk: the halves of columns 16 kb + 4 slot .. + 3
LH_STREAM_H_FN uint32_t stream_h_read_off(uint32_t kc, uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot) {
    return stream_h_granule_off(kc, t * 16u + r16, 2u * kb + (slot >> 1)) + (slot & 1u) * 8u;
}

}  // namespace lh
