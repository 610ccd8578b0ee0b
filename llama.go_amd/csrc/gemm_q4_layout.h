// csrc/gemm_q4_layout.h — where a nibble sits in the weight part of k_gemm_q4b3's LDS ring (kernels_gemm_q4.h): one pure function (no HIP), called by the
// kernel's DMA side AND by its reading side, exported as lh_gemm_q4_w_off and unit-tested without a GPU (tests/test_q4_tiles_cpu.py).
//
// A slab of the tile (32 columns = one quant block) is, per weight row, ONE 16-byte granule of the nibble plane (byte b = column 2 b in the low nibble,
// 2 b + 1 in the high one: kernels_q4.h): [256 rows][16 B] = 4 KB where the int8 kernel stages 8 KB.  Two consecutive slabs (2 p, 2 p + 1) of a row are 32
// contiguous bytes of HBM, and one wave-wide LDS-DMA instruction (lane i lands at base + 16 i) brings them for the wave's own 32 rows: lane i takes row
// i & 31 and source granule i >> 5, so the instruction's 1 KB is [slab parity][32 rows][16 B] - each slab's 512 bytes of a wave stay dense, and the operand
// read of a slab (ds_read_b64 per lane: bytes 8 lh .. 8 lh + 7 of row li's granule) covers exactly those 512 contiguous bytes: every bank twice, the
// minimum for 512 bytes.  (A pair interleaved by row - pitch 32 B - would put a half-wave on 16 banks.)
// The ring holds GEMM_Q4_WPAIRS = 2 slab pairs: pair p lives in slot p & 1 (why two are enough for ring depths 4 and 5: kernels_gemm_q4.h).
//   offset = [pair slot: 8 KB][wave = row >> 5: 1 KB][slab parity: 512 B][row & 31: 16 B][byte]
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_GEMM_Q4_FN __host__ __device__ __forceinline__   // (forced: the kernel carries a target attribute of its own, across which nothing else is inlined)
#else
#define LH_GEMM_Q4_FN inline
#endif

namespace lh {

constexpr uint32_t GEMM_Q4_BM = 256, GEMM_Q4_WPAIRS = 2, GEMM_Q4_WPAIR_BYTES = 2 * GEMM_Q4_BM * 16, GEMM_Q4_W_BYTES = GEMM_Q4_WPAIRS * GEMM_Q4_WPAIR_BYTES;

// byte offset, in the weight part of the ring, of byte `byte` (< 16: columns 2 byte, 2 byte + 1 of the slab) of tile row `row` (< 256) of slab `slab` of the
// work item
LH_GEMM_Q4_FN uint32_t gemm_q4_w_off(uint32_t slab, uint32_t row, uint32_t byte) {
    return ((slab >> 1) % GEMM_Q4_WPAIRS) * GEMM_Q4_WPAIR_BYTES + (row >> 5) * 1024u + (slab & 1u) * 512u + (row & 31u) * 16u + byte;
}
// what lane `lane` of wave `wave`'s DMA instruction for slab pair `pair` moves: tile row, source granule (0 | 1) inside the row's 32 bytes of the pair; its
// 16 bytes land at gemm_q4_w_off(2 pair + granule, row, 0) = (the instruction's base = lane 0's) + 16 lane
LH_GEMM_Q4_FN uint32_t gemm_q4_dma_row(uint32_t wave, uint32_t lane) { return wave * 32u + (lane & 31u); }
LH_GEMM_Q4_FN uint32_t gemm_q4_dma_granule(uint32_t lane) { return lane >> 5; }
// byte offset of the 8 bytes MFMA lane (li = lane & 31, lh = lane >> 5) of wave `wave` reads for slab `slab`: dword st of them = the nibbles of columns
// 16 lh + 8 st .. + 7 of weight row 32 wave + li
LH_GEMM_Q4_FN uint32_t gemm_q4_read_off(uint32_t slab, uint32_t wave, uint32_t li, uint32_t lh) { return gemm_q4_w_off(slab, wave * 32u + li, 8u * lh); }
}  // namespace lh
