// tests/stream_b9w_layout_main.cpp — csrc/stream_b9w_layout.h behind its own main, for a build with -fsanitize=address,undefined
// (tests/test_wide_planes_cpu.py).  stdin: lines "i maxt nct" and "s ncu d F hd".
//   i: the ring image as a heap block of exactly its size: every DMA piece tags the 16 bytes of each lane with what it fetched - every granule exactly once,
//      no two pieces overlap -, every MFMA lane read of both column halves finds the columns it multiplies, and the ring of b9w_nimg images fits 160 KB.
//   s: for every row count 65..128 of a model shape: what the predicate admits has an instantiation for each of the layer's four launches.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "stream_b9w_layout.h"

struct Tag { uint8_t kind, gran; uint16_t row; };

static bool image_ok(uint32_t maxt, uint32_t nct) {
    if (!lh::b9w_built(maxt, nct)) return false;
    const uint32_t size = lh::b9w_image_bytes(maxt, nct);
    std::vector<Tag> img(size / 16, Tag{0xff, 0, 0});
    const int nimg = lh::b9w_nimg((int)maxt, (int)nct, 4);
    bool ok = size == maxt * 4096u + nct * 6144u && lh::b9w_built(maxt, nct) && nimg >= 2 && (uint64_t)nimg * size <= 160u * 1024u;
    for (uint32_t q = 0; q < lh::b9w_pieces(maxt, nct); ++q)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const lh::B9wPiece pc = lh::b9w_piece(maxt, nct, q, lane);
            ok = ok && pc.dst == lh::b9w_piece(maxt, nct, q, 0).dst + 16 * lane && pc.gran < (pc.kind ? 8u : 16u);      // lane-linear: what an LDS-DMA writes
            ok = ok && (pc.kind ? pc.row < nct * 16 : (pc.row < maxt * 16 && (pc.row >> 4) == (q >> 2)));             // a weight piece lies inside one tile
            Tag& t = img.at(pc.dst / 16);
            ok = ok && t.kind == 0xff;                                                                                  // exactly once
            t = Tag{(uint8_t)pc.kind, (uint8_t)pc.gran, (uint16_t)pc.row};
        }
    for (const Tag& t : img) ok = ok && t.kind != 0xff;
    bool tile_seen[8] = {};
    for (uint32_t i = 0; i < 2 * 4 * 16; ++i) {
        const uint32_t kb = i >> 6, slot = (i >> 4) & 3, r16 = i & 15;
        for (uint32_t t = 0; t < maxt; ++t)
            for (uint32_t h = 0; h < 2; ++h) {
                const Tag& g = img.at(lh::b9w_w_read_off(t, r16, kb, slot, h) / 16);
                ok = ok && g.kind == 0 && g.row == t * 16 + r16 && g.gran == kb * 8 + slot * 2 + h;
                ok = ok && lh::b9w_w_read_off(t, r16, kb, slot, h) == ((lh::b9w_w_read_off(0, r16, kb, slot, 0) + t * 4096u) ^ (h ? 16u : 0u));   // the kernel's form
            }
        for (uint32_t half = 0; half < 2; ++half)
            for (uint32_t c = 0; c < lh::b9w_ncw(nct); ++c) {
                const uint32_t ct = lh::b9w_col_tile(nct, half, c);
                ok = ok && ct < nct && (half * lh::b9w_ncw(nct) + c >= nct || ct == half * lh::b9w_ncw(nct) + c);
                tile_seen[ct] = true;
                for (uint32_t p = 0; p < 3; ++p) {
                    const Tag& g = img.at(lh::b9w_x_read_off(maxt, nct, p, ct, r16, kb, slot) / 16);
                    ok = ok && g.kind == 1 + p && g.row == ct * 16 + r16 && g.gran == kb * 4 + slot;
                }
            }
    }
    for (uint32_t ct = 0; ct < nct; ++ct) ok = ok && tile_seen[ct];                                                     // the two halves cover every column tile
    return ok;
}

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'i') {
            unsigned maxt, nct;
            if (scanf("%u %u", &maxt, &nct) != 2) return 2;
            printf("i %u %u %s\n", maxt, nct, image_ok(maxt, nct) ? "ok" : "BAD");
        } else {
            unsigned ncu, d, F, hd, admitted = 0;
            if (scanf("%u %u %u %u", &ncu, &d, &F, &hd) != 4) return 2;
            bool ok = true;
            for (uint32_t n = 1; n <= 200; ++n) {
                const bool adm = lh::b9w_shape_ok(ncu, d, F, hd, n);
                ok = ok && (!adm || (n >= 65 && n <= 128));
                if (!adm) continue;
                ++admitted;
                const lh::B9wLayer l = lh::b9w_layer_maxt(ncu, d, F);
                for (uint32_t m : {l.qkv, l.w13, l.wo, l.w2}) ok = ok && m >= 1 && m <= 8 && image_ok(lh::b9w_maxt_built(m), (n + 15) / 16);
            }
            printf("s %u %u %u %u %s %u\n", ncu, d, F, hd, ok ? "ok" : "BAD", admitted);
        }
    }
    return 0;
}
