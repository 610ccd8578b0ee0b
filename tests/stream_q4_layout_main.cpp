// tests/stream_q4_layout_main.cpp — csrc/stream_q4_layout.h behind its own main, for a build with -fsanitize=address,undefined (tests/
// test_q4_stream_cpu.py starts it as a child process; it is never loaded into Python).  stdin: one case "kc maxt" per line.  Per case the weight part
// of one ring image of k_stream_q4b is filled the way the kernel's DMA pieces fill it - piece q (1 KB = 64 lanes x 16 bytes, lane i at q * 1024 + 16 i) takes
// image rows [q RPW, (q + 1) RPW), lane i the position i % GRW of row q RPW + i / GRW and, through stream_q4_granule_pos, the SOURCE granule stored there -
// into a heap block of EXACTLY maxt * 16 * kc / 2 bytes (a write or read past it is a sanitizer report).  Column c of row r holds the nibble
// (7 r + 3 c + (c >> 4)) & 15.  Then every MFMA lane (tile, r16, quant block, slot) reads its 4 bytes at stream_q4_read_off, must find the nibbles of columns
// 32 kb + 8 slot .. + 7 of its row, and stream_q4_operand of them must be the bf16 of n - 8 of those eight columns in order.  Behind the cases, once: the
// conversion over all 256 byte values and 4096 pseudo-random dwords against (float)(n - 8) computed the plain way.
// stdout, per case: "kc maxt ok" or "kc maxt BAD ...", then "convert ok" or "convert BAD".
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "stream_q4_layout.h"

static uint32_t nib(uint32_t r, uint32_t c) { return (7u * r + 3u * c + (c >> 4)) & 15u; }
static uint16_t bf16_of(int q) {
    const float f = (float)q;
    uint32_t b;
    memcpy(&b, &f, 4);
    return (uint16_t)(b >> 16);
}
static bool operand_ok(uint32_t v) {
    uint32_t o[4];
    lh::stream_q4_operand(v, o);
    for (uint32_t k = 0; k < 8; ++k) {
        const uint16_t got = (uint16_t)(o[k >> 1] >> (16 * (k & 1)));
        if (got != bf16_of((int)((v >> (4 * k)) & 15u) - 8)) return false;
    }
    return true;
}

int main() {
    unsigned kc, maxt;
    while (scanf("%u %u", &kc, &maxt) == 2) {
        if ((kc != 128 && kc != 256 && kc != 512) || maxt < 1 || maxt > 8) { printf("%u %u BAD arguments\n", kc, maxt); continue; }
        const uint32_t grw = kc / 32, rpw = 64 / grw, rows = maxt * 16, bytes = rows * (kc / 2);
        uint8_t* img = new uint8_t[bytes];
        std::vector<uint8_t> hit(bytes / 16, 0);
        bool ok = true;
        for (uint32_t q = 0; q < rows / rpw && ok; ++q)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t r = q * rpw + lane / grw, gd = lane % grw, gs = lh::stream_q4_granule_pos(kc, r, gd);
                const uint32_t dst = q * 1024u + lane * 16u;
                if (gs >= grw || dst != lh::stream_q4_granule_off(kc, r, gs) || hit[dst / 16]) { ok = false; break; }   // lane-linear destination = the layout's offset
                hit[dst / 16] = 1;
                uint8_t v[16];
                for (uint32_t b = 0; b < 16; ++b) v[b] = (uint8_t)(nib(r, gs * 32 + 2 * b) | nib(r, gs * 32 + 2 * b + 1) << 4);
                memcpy(img + dst, v, 16);
            }
        for (uint32_t i = 0; i < bytes / 16 && ok; ++i) ok = hit[i] == 1;   // a bijection: every granule position written once
        for (uint32_t t = 0; t < maxt && ok; ++t)
            for (uint32_t r16 = 0; r16 < 16 && ok; ++r16)
                for (uint32_t kb = 0; kb < kc / 32 && ok; ++kb)
                    for (uint32_t slot = 0; slot < 4; ++slot) {
                        uint32_t v, o[4];
                        memcpy(&v, img + lh::stream_q4_read_off(kc, t, r16, kb, slot), 4);
                        lh::stream_q4_operand(v, o);
                        for (uint32_t e = 0; e < 8; ++e) {
                            const uint32_t n = nib(t * 16 + r16, 32 * kb + 8 * slot + e);
                            ok = ok && ((v >> (4 * e)) & 15u) == n && (uint16_t)(o[e >> 1] >> (16 * (e & 1))) == bf16_of((int)n - 8);
                        }
                    }
        printf("%u %u %s\n", kc, maxt, ok ? "ok" : "BAD layout");
        delete[] img;
    }
    bool cv = true;
    for (uint32_t b = 0; b < 256 && cv; ++b) cv = operand_ok(b * 0x01010101u) && operand_ok(b) && operand_ok(b << 24);
    uint32_t x = 0x9e3779b9u;
    for (int i = 0; i < 4096 && cv; ++i) { x = x * 1664525u + 1013904223u; cv = operand_ok(x); }
    printf("convert %s\n", cv ? "ok" : "BAD");
    return 0;
}
