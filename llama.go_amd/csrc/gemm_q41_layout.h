// csrc/gemm_q41_layout.h — where the bytes of k_gemm_b9_q41's LDS ring sit (kernels_gemm_q41.h): pure functions (no HIP), called by the kernel's DMA side
// AND by its reading side, exported as lh_gemm_q41_piece / lh_gemm_q41_read_off and unit-tested without a GPU (tests/test_q41_tiles_cpu.py).
//
// The stage.  [3 planes][128 rows][32 bf16] of X (k_gemm_b9's slab with its swizzle, 24 KB) | [256 rows][16 B] of nibbles (4 KB): 28 KB.  A slab of the
// tile (32 columns) is ONE Q4_1 block per weight row = one 16-byte granule of the nibble plane (byte b = column 2 b in the low nibble, 2 b + 1 in the high
// one: kernels_q41.h), so a wave-wide LDS-DMA instruction (lane i lands at base + 16 i) brings 64 rows: nibble piece q (0..3) = tile rows 64 q .. 64 q + 63,
// row r at W_OFF + 16 r, no swizzle - the 32 rows of an MFMA wave are 512 dense bytes and one ds_read_b128 per lane covers them (both halves of the wave
// read the same 32 addresses).
// The pair ring.  The (d, m) of a row's two consecutive blocks (2 P, 2 P + 1) are 16 contiguous bytes of the pair plane [M][K / 32][2]: pair piece q = tile
// rows 64 q .. of slab pair P, row r at 16 r of slot P % slots; (d, m) of the block of parity h at + 8 h.  P counts ABSOLUTE slabs of the matrix, so a
// split-K range that begins at an odd slab finds its first block in the second half of its first pair.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_GEMM_Q41_FN __host__ __device__ inline
#else
#define LH_GEMM_Q41_FN inline
#endif

namespace lh {

constexpr uint32_t GQ41_BN = 128, GQ41_BM = 256, GQ41_XP_BYTES = GQ41_BN * 64, GQ41_W_OFF = 3 * GQ41_XP_BYTES, GQ41_STAGE = GQ41_W_OFF + GQ41_BM * 16;
constexpr uint32_t GQ41_PAIR_BYTES = GQ41_BM * 16;
// slots of the pair ring for a stage ring of depth nst (why these suffice: kernels_gemm_q41.h)
LH_GEMM_Q41_FN constexpr uint32_t gemm_q41_pair_slots(uint32_t nst) { return nst / 2 + 1; }
LH_GEMM_Q41_FN constexpr uint32_t gemm_q41_lds_bytes(uint32_t nst) { return nst * GQ41_STAGE + gemm_q41_pair_slots(nst) * GQ41_PAIR_BYTES; }

// nibble or pair piece q (0..3), lane (0..63): the tile row the lane fetches 16 bytes of, and where they land - in the stage (nibbles) or in the pair slot
LH_GEMM_Q41_FN uint32_t gemm_q41_piece_row(uint32_t q, uint32_t lane) { return q * 64u + lane; }
LH_GEMM_Q41_FN uint32_t gemm_q41_nib_dst(uint32_t q, uint32_t lane) { return GQ41_W_OFF + q * 1024u + lane * 16u; }
LH_GEMM_Q41_FN uint32_t gemm_q41_pair_dst(uint32_t q, uint32_t lane) { return q * 1024u + lane * 16u; }
// the pair slot of the block of absolute slab `slab`
LH_GEMM_Q41_FN uint32_t gemm_q41_pair_slot(uint32_t slab, uint32_t nst) { return (slab >> 1) % gemm_q41_pair_slots(nst); }
// byte offset in the stage of the 16 nibble bytes MFMA lane li (0..31: weight row 32 wave + li) reads per slab; k-step kk of lane half lh uses dword
// gemm_q41_frag_dword of them = bytes 8 kk + 4 lh .. + 3 = slab columns 16 kk + 8 lh .. + 7
LH_GEMM_Q41_FN uint32_t gemm_q41_w_read_off(uint32_t wave, uint32_t li) { return GQ41_W_OFF + (wave * 32u + li) * 16u; }
LH_GEMM_Q41_FN uint32_t gemm_q41_frag_dword(uint32_t kk, uint32_t lh) { return 2u * kk + lh; }
// byte offset in a pair slot of the row's 16 bytes (d0, m0, d1, m1)
LH_GEMM_Q41_FN uint32_t gemm_q41_pair_read_off(uint32_t wave, uint32_t li) { return (wave * 32u + li) * 16u; }

}  // namespace lh
