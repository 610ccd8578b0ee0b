// csrc/stream_b9h_layout.h — where the bytes of a ring image of k_stream_b9_h (kernels_stream_b9_h.h) sit, and which bf16 products it issues: pure
// functions (no HIP), called by the kernel's loader waves AND by its MFMA waves, exported as lh_stream_b9h_piece / lh_stream_b9h_read_off /
// lh_stream_b9h_product and unit-tested without a GPU (tests/test_f16_planes_cpu.py, tests/stream_b9h_layout_main.cpp).
//
// Image of one 64-column chunk: weights [maxt * 16 rows][64 halves] | planes [3][nct * 16 rows][64 bf16] - 128-byte rows everywhere, eight 16-byte granules
// per row (granule g = columns 8 g .. 8 g + 7 of the chunk).  An LDS-DMA instruction writes lane i at piece base + 16 i, so a 1 KB piece is eight rows and
// the permutation that keeps the operand reads conflict-free goes on the SOURCE address: granule g of image row r is STORED at position g ^ ((r >> 1) & 7)
// (two rows per bank line; k_stream_b9's plane swizzle, for weights and planes alike), an involution in g, so the loader - which picks the source granule
// for the position its lane lands on - and the reader use the same function.
// Pieces of a chunk: 2 maxt weight pieces (piece q: image rows 8 q .. 8 q + 7, inside the 16-row tile slot q >> 1), then 3 * 2 nct plane pieces (plane by
// plane).  Four loader waves: piece 4 j + wave in slot j, surplus slots repeat the last piece.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_B9H_FN __host__ __device__ inline
#else
#define LH_B9H_FN inline
#endif

namespace lh {

LH_B9H_FN constexpr uint32_t b9h_w_bytes(uint32_t maxt) { return maxt * 2048u; }
LH_B9H_FN constexpr uint32_t b9h_plane_bytes(uint32_t nct) { return nct * 2048u; }
LH_B9H_FN constexpr uint32_t b9h_image_bytes(uint32_t maxt, uint32_t nct) { return b9h_w_bytes(maxt) + 3u * b9h_plane_bytes(nct); }
LH_B9H_FN constexpr uint32_t b9h_pieces(uint32_t maxt, uint32_t nct) { return 2u * maxt + 6u * nct; }
// images in the ring: as many as fit into 160 KB, up to cap
LH_B9H_FN constexpr int b9h_nimg(int maxt, int nct, int cap) {
    const int n = (int)(160u * 1024u / b9h_image_bytes((uint32_t)maxt, (uint32_t)nct));
    return n < cap ? n : cap;
}
// position of granule g in its row r (and the granule found at position g)
LH_B9H_FN constexpr uint32_t b9h_granule_pos(uint32_t r, uint32_t g) { return g ^ ((r >> 1) & 7u); }

// DMA piece q (< b9h_pieces), lane (< 64): where the lane's 16 bytes land and what they are
struct B9hPiece {
    uint32_t dst;    // byte offset in the image
    uint32_t kind;   // 0: weights, 1 + p: plane p (0 hi, 1 mid, 2 lo)
    uint32_t row;    // weights: image row (tile slot row >> 4, weight row row & 15 of it); planes: activation row
    uint32_t gran;   // source granule of the row's 128 chunk bytes
};
LH_B9H_FN constexpr B9hPiece b9h_piece(uint32_t maxt, uint32_t nct, uint32_t q, uint32_t lane) {
    const uint32_t nwi = 2u * maxt, nxp = 2u * nct;
    if (q < nwi) {
        const uint32_t rr = q * 8u + (lane >> 3);
        return B9hPiece{q * 1024u + lane * 16u, 0u, rr, b9h_granule_pos(rr, lane & 7u)};
    }
    const uint32_t xq = q - nwi, p = xq / nxp, xi = xq - p * nxp, rr = xi * 8u + (lane >> 3);
    return B9hPiece{b9h_w_bytes(maxt) + p * b9h_plane_bytes(nct) + xi * 1024u + lane * 16u, 1u + p, rr, b9h_granule_pos(rr, lane & 7u)};
}
// byte offset, in the weight part of the image, of the 16 bytes MFMA lane (r16, slot) reads of tile slot t for k-block kb: the eight halves of chunk
// columns 32 kb + 8 slot .. + 7 of weight row r16 - ONE ds_read_b128
LH_B9H_FN constexpr uint32_t b9h_w_read_off(uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot) {
    const uint32_t r = t * 16u + r16;
    return r * 128u + b9h_granule_pos(r, kb * 4u + slot) * 16u;
}
// ... and, in the image, of the same columns of activation row 16 ct + r16 of plane p
LH_B9H_FN constexpr uint32_t b9h_x_read_off(uint32_t maxt, uint32_t nct, uint32_t p, uint32_t ct, uint32_t r16, uint32_t kb, uint32_t slot) {
    const uint32_t r = ct * 16u + r16;
    return b9h_w_bytes(maxt) + p * b9h_plane_bytes(nct) + r * 128u + b9h_granule_pos(r, kb * 4u + slot) * 16u;
}

// Product i of nprod (8 | 6): the activation plane and the weight part it multiplies (0 hi, 1 mid, 2 lo).  Eight: k_stream_b9's list at B9S_PRODUCTS = 8,
//     (xl,wm) (xm,wl) (xl,wh) (xm,wm) (xh,wl) (xm,wh) (xh,wm) (xh,wh);
// six: the same without the two products of the weights' lo part (+0 for every finite half), in the same order.
LH_B9H_FN constexpr int b9h_product_x(int nprod, int i) {
    constexpr int PX8[8] = {2, 1, 2, 1, 0, 1, 0, 0}, PX6[6] = {2, 2, 1, 1, 0, 0};
    return nprod == 6 ? PX6[i] : PX8[i];
}
LH_B9H_FN constexpr int b9h_product_w(int nprod, int i) {
    constexpr int PW8[8] = {1, 2, 0, 1, 2, 0, 1, 0}, PW6[6] = {1, 0, 1, 0, 1, 0};
    return nprod == 6 ? PW6[i] : PW8[i];
}

}  // namespace lh
