// tests/stream_f16_layout_main.cpp — csrc/stream_f16_layout.h behind its own main, for a build with -fsanitize=address,undefined (tests/
// test_f16_stream_cpu.py starts it as a child process; it is never loaded into Python).  stdin: one case "kc maxt" per line.  Per case the weight part
// of one ring image of k_stream_dma_h is filled the way the loader waves fill it - piece q (1 KB = 64 lanes x 16 bytes, lane i at q * 1024 + 16 i) takes
// image rows [q RPW, (q + 1) RPW), lane i the position i % GRW of row q RPW + i / GRW and, through stream_h_granule_pos, the SOURCE granule stored there -
// into a heap block of EXACTLY maxt * 16 * kc * 2 bytes (a write or read past it is a sanitizer report), every half tagged (row << 8 | column).  Then
// every MFMA lane (tile, r16, k-block, slot) reads its 8 bytes at stream_h_read_off and must find the halves of columns 16 kb + 4 slot .. + 3 of its row.
// stdout, per case: "kc maxt ok" or "kc maxt BAD ...".
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "stream_f16_layout.h"

int main() {
    unsigned kc, maxt;
    while (scanf("%u %u", &kc, &maxt) == 2) {
        if ((kc != 64 && kc != 128) || maxt < 1 || maxt > 8) { printf("%u %u BAD arguments\n", kc, maxt); continue; }
        const uint32_t grw = kc / 8, rpw = 64 / grw, rows = maxt * 16, bytes = rows * kc * 2;
        uint8_t* img = new uint8_t[bytes];
        std::vector<uint8_t> hit(bytes / 16, 0);
        bool ok = true;
        for (uint32_t q = 0; q < rows / rpw && ok; ++q)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t r = q * rpw + lane / grw, gd = lane % grw, gs = lh::stream_h_granule_pos(kc, r, gd);
                const uint32_t dst = q * 1024u + lane * 16u;
                if (gs >= grw || dst != lh::stream_h_granule_off(kc, r, gs) || hit[dst / 16]) { ok = false; break; }   // lane-linear destination = the layout's offset
                hit[dst / 16] = 1;
                uint16_t v[8];
                for (uint32_t e = 0; e < 8; ++e) v[e] = (uint16_t)(r << 8 | (gs * 8 + e));
                memcpy(img + dst, v, 16);
            }
        for (uint32_t i = 0; i < bytes / 16 && ok; ++i) ok = hit[i] == 1;   // a bijection: every granule position written once
        for (uint32_t t = 0; t < maxt && ok; ++t)
            for (uint32_t r16 = 0; r16 < 16 && ok; ++r16)
                for (uint32_t kb = 0; kb < kc / 16 && ok; ++kb)
                    for (uint32_t slot = 0; slot < 4; ++slot) {
                        uint16_t v[4];
                        memcpy(v, img + lh::stream_h_read_off(kc, t, r16, kb, slot), 8);
                        for (uint32_t e = 0; e < 4; ++e) ok = ok && v[e] == (uint16_t)((t * 16 + r16) << 8 | (16 * kb + 4 * slot + e));
                    }
        printf("%u %u %s\n", kc, maxt, ok ? "ok" : "BAD layout");
        delete[] img;
    }
    return 0;
}
