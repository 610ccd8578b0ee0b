// csrc/stream_b9w_layout.h — k_stream_b9w (kernels_stream_b9w.h): where the bytes of a ring image sit, which column tiles an MFMA wave owns, which
// (row tiles, column tiles) shapes are built and which model shapes the host sends there.  Pure functions (no HIP), called by the kernel's loader
// waves, by its MFMA waves and by plan.hip, and unit-tested without a GPU (tests/test_wide_planes_cpu.py, tests/stream_b9w_layout_main.cpp).
//
// Image of one 64-column chunk: weights [maxt * 16 rows][64 floats] (256-byte rows, sixteen 16-byte granules) | planes [3][nct * 16 rows][64 bf16]
// (128-byte rows, eight granules).  An LDS-DMA instruction writes lane i at piece base + 16 i, so a 1 KB piece is four weight rows or eight plane rows
// and the permutation that keeps the operand reads conflict-free goes on the SOURCE address:
//   weights: granule g of image row r is STORED at position g ^ (r & 15) (k_stream_dma's and k_stream_b9's swizzle).  An MFMA lane (r16, slot) reads
//     the two granules 8 kb + 2 slot, + 1 of row 16 t + r16.  256-byte rows all start on bank 0, so the position alone decides the banks; a ds_read_b128
//     lane group - eight rows at slot s, eight at slot s ^ 1 - touches sixteen different positions;
//   planes: granule g of row r at g ^ ((r >> 1) & 7) (k_stream_b9's): two 128-byte rows make one bank line, rows 2 i and 2 i + 1 share the permutation
//     and lie in different halves of the line, so sixteen lanes cover all sixteen granule slots of the 2 x 8.
// Both are involutions in g: the loader - which picks the source granule for the position its lane lands on - and the reader use the same function.
// Pieces of a chunk: 4 maxt weight pieces (piece q: image rows 4 q .. 4 q + 3, inside tile slot q >> 2), then 3 * 2 nct plane pieces (plane by plane).
// Four loader waves: piece 4 j + wave in slot j, surplus slots repeat the last piece.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_B9W_FN __host__ __device__ inline
#else
#define LH_B9W_FN inline
#endif

namespace lh {

constexpr uint32_t B9W_MIN_ROWS = 65, B9W_MAX_ROWS = 128, B9W_LDS_BYTES = 160u * 1024u;

LH_B9W_FN constexpr uint32_t b9w_w_bytes(uint32_t maxt) { return maxt * 4096u; }
LH_B9W_FN constexpr uint32_t b9w_plane_bytes(uint32_t nct) { return nct * 2048u; }
LH_B9W_FN constexpr uint32_t b9w_image_bytes(uint32_t maxt, uint32_t nct) { return b9w_w_bytes(maxt) + 3u * b9w_plane_bytes(nct); }
LH_B9W_FN constexpr uint32_t b9w_pieces(uint32_t maxt, uint32_t nct) { return 4u * maxt + 6u * nct; }
// images in the ring: as many as fit into 160 KB, up to cap
LH_B9W_FN constexpr int b9w_nimg(int maxt, int nct, int cap) {
    const int n = (int)(B9W_LDS_BYTES / b9w_image_bytes((uint32_t)maxt, (uint32_t)nct));
    return n < cap ? n : cap;
}
LH_B9W_FN constexpr uint32_t b9w_w_pos(uint32_t r, uint32_t g) { return g ^ (r & 15u); }
LH_B9W_FN constexpr uint32_t b9w_x_pos(uint32_t r, uint32_t g) { return g ^ ((r >> 1) & 7u); }

// DMA piece q (< b9w_pieces), lane (< 64): where the lane's 16 bytes land and what they are
struct B9wPiece {
    uint32_t dst;    // byte offset in the image
    uint32_t kind;   // 0: weights, 1 + p: plane p (0 hi, 1 mid, 2 lo)
    uint32_t row;    // weights: image row (tile slot row >> 4, weight row row & 15 of it); planes: activation row
    uint32_t gran;   // source granule of the row's chunk bytes
};
LH_B9W_FN constexpr B9wPiece b9w_piece(uint32_t maxt, uint32_t nct, uint32_t q, uint32_t lane) {
    const uint32_t nwi = 4u * maxt, nxp = 2u * nct;
    if (q < nwi) {
        const uint32_t rr = q * 4u + (lane >> 4);
        return B9wPiece{q * 1024u + lane * 16u, 0u, rr, b9w_w_pos(rr, lane & 15u)};
    }
    const uint32_t xq = q - nwi, p = xq / nxp, xi = xq - p * nxp, rr = xi * 8u + (lane >> 3);
    return B9wPiece{b9w_w_bytes(maxt) + p * b9w_plane_bytes(nct) + xi * 1024u + lane * 16u, 1u + p, rr, b9w_x_pos(rr, lane & 7u)};
}
// byte offset, in the weight part of the image, of half h (0 | 1) of the fragment MFMA lane (r16, slot) reads of tile slot t for k-block kb: the four
// floats of chunk columns 32 kb + 8 slot + 4 h .. + 3 of weight row r16
LH_B9W_FN constexpr uint32_t b9w_w_read_off(uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot, uint32_t h) {
    const uint32_t r = t * 16u + r16;
    return r * 256u + b9w_w_pos(r, kb * 8u + slot * 2u + h) * 16u;
}
// ... and, in the image, of the eight bf16 of the same columns of activation row 16 ct + r16 of plane p
LH_B9W_FN constexpr uint32_t b9w_x_read_off(uint32_t maxt, uint32_t nct, uint32_t p, uint32_t ct, uint32_t r16, uint32_t kb, uint32_t slot) {
    const uint32_t r = ct * 16u + r16;
    return b9w_w_bytes(maxt) + p * b9w_plane_bytes(nct) + r * 128u + b9w_x_pos(r, kb * 4u + slot) * 16u;
}

// The four MFMA waves are 2 k-blocks x 2 column halves.  A half holds ncw = ceil(nct / 2) column tiles; with an odd count the second half's last slot
// repeats column tile nct - 1 (its sums land in token columns >= 16 nct >= n, which the epilogue never emits).
LH_B9W_FN constexpr uint32_t b9w_ncw(uint32_t nct) { return (nct + 1u) / 2u; }
LH_B9W_FN constexpr uint32_t b9w_col_tile(uint32_t nct, uint32_t half, uint32_t c) {
    const uint32_t ct = half * b9w_ncw(nct) + c;
    return ct < nct ? ct : nct - 1u;
}

// (row tiles per workgroup, column tiles) with an instantiation: the row-tile counts of the stream kernels (1, 2, 3, 4, 6, 8) next to 5..8 column
// tiles, where two images fit the LDS.  launch_stream_b9w (plan.hip) answers "not applicable" for every other pair.
LH_B9W_FN constexpr bool b9w_built(uint32_t maxt, uint32_t nct) {
    return (maxt == 1 || maxt == 2 || maxt == 3 || maxt == 4 || maxt == 6 || maxt == 8) && nct >= 5 && nct <= 8 && b9w_nimg((int)maxt, (int)nct, 4) >= 2;
}
LH_B9W_FN constexpr uint32_t b9w_maxt_built(uint32_t maxt) { return maxt <= 4 ? maxt : (maxt <= 6 ? 6u : (maxt <= 8 ? 8u : 0u)); }
// K-split of wo / w2 (q8b_split_groups, plan.hip): fours, halved while a workgroup's share of the contraction would fall under two chunks
LH_B9W_FN constexpr uint32_t b9w_split_groups(uint32_t nchunks, uint32_t ncu) {
    uint32_t S = 4;
    while (S > 1 && (nchunks < 2 * S || ncu / S == 0)) S >>= 1;
    return S;
}
// Row tiles of the busiest workgroup in each of a layer's four launches: wq|wk|wv, w1|w3 (pairs), wo and w2 (K-split)
struct B9wLayer { uint32_t qkv, w13, wo, w2; };
LH_B9W_FN constexpr B9wLayer b9w_layer_maxt(uint32_t ncu, uint32_t d, uint32_t F) {
    const uint32_t go = ncu / b9w_split_groups(d / 64u, ncu), g2 = ncu / b9w_split_groups(F / 64u, ncu);
    return B9wLayer{(3u * d / 16u + ncu - 1u) / ncu, 2u * ((F / 16u + ncu - 1u) / ncu), (d / 16u + go - 1u) / go, (d / 16u + g2 - 1u) / g2};
}
// An Eval of n rows of an fp32 model (embd d, ff F, head size hd) on ncu compute units has every layer launch on k_stream_b9w
LH_B9W_FN constexpr bool b9w_shape_ok(uint32_t ncu, uint32_t d, uint32_t F, uint32_t hd, uint32_t n) {
    if (ncu < 4 || n < B9W_MIN_ROWS || n > B9W_MAX_ROWS || d == 0 || d > 8192 || d % 128 || F == 0 || F % 128 || hd == 0 || hd % 4 || d % hd) return false;
    const B9wLayer l = b9w_layer_maxt(ncu, d, F);
    const uint32_t nct = (n + 15u) / 16u;
    return b9w_built(b9w_maxt_built(l.qkv), nct) && b9w_built(b9w_maxt_built(l.w13), nct) && b9w_built(b9w_maxt_built(l.wo), nct) && b9w_built(b9w_maxt_built(l.w2), nct);
}

}  // namespace lh
