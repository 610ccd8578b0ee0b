// tests/gemm_f16_split_main.cpp — csrc/gemm_f16_layout.h behind its own main, for a build with -fsanitize=address,undefined (tests/test_f16_tiles_cpu.py
// starts it as a child process; it is never loaded into Python).  No input.
//   1. gemm_h_split over all 65 536 half patterns: for every finite one the widened value w, hi = w's top 16 bits, r1 = w - hi; r1's low 16 bits are 0 (so
//      mid = r1 and the third part r1 - mid is +0), hi + mid == w exactly, every non-zero part has a magnitude >= 2^-100 (the smallest is 2^-24).
//   2. one ring stage of k_gemm_b9_h, a heap block of EXACTLY GH_STAGE bytes (a write or read past it is a sanitizer report): the 40 DMA pieces x 64 lanes
//      write their 16 bytes where the loader does, every 16-byte unit exactly once, tagged (is W, plane, row, source granule); then every lane of every wave
//      reads its weight fragment of both k-steps at gemm_h_w_read_off and must find granule 2 kk + lh of its row.
// stdout: "split ok <smallest non-zero part's exponent>" / "layout ok", or a line starting with BAD.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "gemm_f16_layout.h"

static float as_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main() {
    int min_exp = 1000;
    for (uint32_t h = 0; h < 65536; ++h) {
        uint32_t wb = 1, r1b = 1;
        lh::gemm_h_split((uint16_t)h, &wb, &r1b);
        if (((h >> 10) & 31u) == 31u) continue;                       // inf / NaN: outside the contract
        const float w = as_float(wb), hi = as_float(wb & 0xffff0000u), r1 = as_float(r1b);
        const float mid = as_float(r1b & 0xffff0000u), lo = r1 - mid;
        const bool neg = (h & 0x8000u) != 0;
        const double want = ldexp((double)(h & 0x3ffu) + (((h >> 10) & 31u) ? 1024.0 : 0.0), (int)(((h >> 10) & 31u) ? ((h >> 10) & 31u) : 1u) - 25) * (neg ? -1.0 : 1.0);
        if ((double)w != want || (want == 0.0 && wb != ((uint32_t)neg << 31))) { printf("BAD widen %04x\n", h); return 1; }
        if ((r1b & 0xffffu) || as_bits(lo) != 0u || hi + mid != w || as_bits(w - hi) != r1b) { printf("BAD split %04x\n", h); return 1; }
        const float parts[2] = {hi, mid};
        for (float p : parts)
            if (p != 0.f) {
                int e;
                frexpf(fabsf(p), &e);
                if (e - 1 < min_exp) min_exp = e - 1;
                if (fabsf(p) < ldexpf(1.f, -100)) { printf("BAD small part %04x\n", h); return 1; }
            }
    }
    printf("split ok %d\n", min_exp);

    uint32_t* stage = new uint32_t[lh::GH_STAGE / 4];
    std::vector<uint8_t> hit(lh::GH_STAGE / 16, 0);
    for (uint32_t p = 0; p < lh::GH_PIECES; ++p)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t dst = lh::gemm_h_piece_dst(p, lane), row = lh::gemm_h_piece_row(p, lane), gs = lh::gemm_h_piece_granule(p, lane);
            const bool is_w = p >= lh::GH_XPIECES;
            if (dst % 16 || dst + 16 > lh::GH_STAGE || gs > 3 || row >= (is_w ? lh::GH_BM : lh::GH_BN) || hit[dst / 16]) { printf("BAD piece %u %u\n", p, lane); return 1; }
            hit[dst / 16] = 1;
            const uint32_t tag = (uint32_t)is_w << 24 | (is_w ? 0u : p / 8u) << 16 | row << 4 | gs;
            for (int e = 0; e < 4; ++e) stage[dst / 4 + e] = tag;
            // the piece's destination is the layout's: position gemm_h_granule_pos(row, gs) of the row
            const uint32_t base = is_w ? lh::GH_W_OFF : (p / 8u) * lh::GH_XP_BYTES;
            if (dst != base + row * 64u + lh::gemm_h_granule_pos(row, gs) * 16u) { printf("BAD place %u %u\n", p, lane); return 1; }
        }
    for (uint32_t i = 0; i < lh::GH_STAGE / 16; ++i)
        if (hit[i] != 1) { printf("BAD cover %u\n", i); return 1; }
    for (uint32_t wm = 0; wm < 8; ++wm)
        for (uint32_t li = 0; li < 32; ++li)
            for (uint32_t lh = 0; lh < 2; ++lh)
                for (uint32_t kk = 0; kk < 2; ++kk) {
                    const uint32_t off = lh::gemm_h_w_read_off(wm, li, lh, kk);
                    uint32_t v[4];
                    memcpy(v, (const char*)stage + off, 16);
                    const uint32_t want = 1u << 24 | (wm * 32u + li) << 4 | (2u * kk + lh);
                    if (off % 16 || v[0] != want || v[3] != want) { printf("BAD read %u %u %u %u\n", wm, li, lh, kk); return 1; }
                }
    delete[] stage;
    printf("layout ok\n");
    return 0;
}
