// tests/stream_b9h_layout_main.cpp — csrc/stream_b9h_layout.h behind its own main, for a build with -fsanitize=address,undefined
// (tests/test_f16_planes_cpu.py).  stdin: lines "maxt nct"; per line the ring image as a heap block of exactly its size: every DMA piece tags the 16
// bytes of each lane with what it fetched, every granule exactly once, and every MFMA lane read finds the columns it multiplies.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "stream_b9h_layout.h"

struct Tag { uint8_t kind, gran; uint16_t row; };

int main() {
    unsigned maxt, nct;
    while (scanf("%u %u", &maxt, &nct) == 2) {
        const uint32_t size = lh::b9h_image_bytes(maxt, nct);
        std::vector<Tag> img(size / 16, Tag{0xff, 0, 0});
        bool ok = size == maxt * 2048u + nct * 6144u;
        for (uint32_t q = 0; q < lh::b9h_pieces(maxt, nct); ++q)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const lh::B9hPiece pc = lh::b9h_piece(maxt, nct, q, lane);
                ok = ok && pc.dst == lh::b9h_piece(maxt, nct, q, 0).dst + 16 * lane && pc.gran < 8;      // lane-linear: what an LDS-DMA writes
                ok = ok && (pc.kind ? pc.row < nct * 16 : (pc.row < maxt * 16 && (pc.row >> 4) == (q >> 1)));
                Tag& t = img.at(pc.dst / 16);
                ok = ok && t.kind == 0xff;                                                               // exactly once
                t = Tag{(uint8_t)pc.kind, (uint8_t)pc.gran, (uint16_t)pc.row};
            }
        for (const Tag& t : img) ok = ok && t.kind != 0xff;
        for (uint32_t i = 0; i < 2 * 4 * 16; ++i) {
            const uint32_t kb = i >> 6, slot = (i >> 4) & 3, r16 = i & 15;
            for (uint32_t t = 0; t < maxt; ++t) {
                const Tag& g = img.at(lh::b9h_w_read_off(t, r16, kb, slot) / 16);
                ok = ok && g.kind == 0 && g.row == t * 16 + r16 && g.gran == kb * 4 + slot;
            }
            for (uint32_t pc = 0; pc < 3 * nct; ++pc) {
                const Tag& g = img.at(lh::b9h_x_read_off(maxt, nct, pc / nct, pc % nct, r16, kb, slot) / 16);
                ok = ok && g.kind == 1 + pc / nct && g.row == (pc % nct) * 16 + r16 && g.gran == kb * 4 + slot;
            }
        }
        printf("%u %u %s\n", maxt, nct, ok ? "ok" : "BAD");
    }
    return 0;
}
