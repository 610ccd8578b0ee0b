// csrc/stream_b9wh_layout.h — k_stream_b9w_h (kernels_stream_b9w_h.h): where the bytes of a ring image sit, how deep the ring is and which (row tiles,
// column tiles) shapes are built.  Pure functions (no HIP), called by the kernel's loader waves, by its MFMA waves and by plan.hip, exported as
// lh_stream_b9wh_piece / lh_stream_b9wh_read_off and unit-tested without a GPU (tests/test_f16_wide_planes_cpu.py).
//
// Image of one 64-column chunk: weights [maxt * 16 rows][64 halves] | planes [3][nct * 16 rows][64 bf16] - 128-byte rows everywhere, eight 16-byte
// granules per row, granule g of image row r STORED at position g ^ ((r >> 1) & 7): the geometry, the source-side swizzle and the 1 KB pieces (eight
// weight rows of one tile; eight plane rows) of stream_b9h_layout.h, whose functions take any tile counts - here five to eight column tiles.  The planes
// follow the weights plane by plane as in stream_b9w_layout.h.  Which column tiles an MFMA wave owns (b9w_ncw, b9w_col_tile) and which model shapes the
// host sends here (b9w_shape_ok) are stream_b9w_layout.h's; the products are stream_b9h_layout.h's (b9h_product_x / b9h_product_w).
#pragma once
#include "stream_b9h_layout.h"
#include "stream_b9w_layout.h"

namespace lh {

LH_B9H_FN constexpr uint32_t b9wh_w_bytes(uint32_t maxt) { return b9h_w_bytes(maxt); }
LH_B9H_FN constexpr uint32_t b9wh_plane_bytes(uint32_t nct) { return b9h_plane_bytes(nct); }
LH_B9H_FN constexpr uint32_t b9wh_image_bytes(uint32_t maxt, uint32_t nct) { return b9wh_w_bytes(maxt) + 3u * b9wh_plane_bytes(nct); }   // maxt 2048 + nct 6144
LH_B9H_FN constexpr uint32_t b9wh_pieces(uint32_t maxt, uint32_t nct) { return 2u * maxt + 6u * nct; }
// images in the ring: as many as fit into 160 KB, up to cap.  No part of the sums: (6, 6) holds three where the fp32 kernel holds two.
LH_B9H_FN constexpr int b9wh_nimg(int maxt, int nct, int cap) {
    const int n = (int)(B9W_LDS_BYTES / b9wh_image_bytes((uint32_t)maxt, (uint32_t)nct));
    return n < cap ? n : cap;
}
// DMA piece q (< b9wh_pieces), lane (< 64): where the lane's 16 bytes land and what they are (weight piece q: image rows 8 q .. 8 q + 7 of tile slot q >> 1)
LH_B9H_FN constexpr B9hPiece b9wh_piece(uint32_t maxt, uint32_t nct, uint32_t q, uint32_t lane) { return b9h_piece(maxt, nct, q, lane); }
// byte offset in the image of the eight halves of chunk columns 32 kb + 8 slot .. + 7 of weight row r16 of tile slot t: ONE ds_read_b128 (tile slot t: + 2048 t)
LH_B9H_FN constexpr uint32_t b9wh_w_read_off(uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot) { return b9h_w_read_off(t, r16, kb, slot); }
// ... and of the eight bf16 of the same columns of activation row 16 ct + r16 of plane p
LH_B9H_FN constexpr uint32_t b9wh_x_read_off(uint32_t maxt, uint32_t nct, uint32_t p, uint32_t ct, uint32_t r16, uint32_t kb, uint32_t slot) {
    return b9h_x_read_off(maxt, nct, p, ct, r16, kb, slot);
}
// The fp32 predicate decides although halves would fit more: an f16 model never takes a launch its widened twin does not.
LH_B9H_FN constexpr bool b9wh_built(uint32_t maxt, uint32_t nct) { return b9w_built(maxt, nct); }

// The hand schedule of an MFMA wave: behind MFMA m >= s0 of a tile's nmt stand pieces [(m - s0) npc / (nmt - s0), (m - s0 + 1) npc / (nmt - s0)) of the
// next fragment's npc.  -> how many pieces a tile issues (the kernel asserts: all of them)
LH_B9H_FN constexpr int b9wh_pieces_issued(int nmt, int s0, int npc) {
    int n = 0;
    for (int m = s0; m < nmt; ++m) n += (m - s0 + 1) * npc / (nmt - s0) - (m - s0) * npc / (nmt - s0);
    return n;
}

}  // namespace lh
