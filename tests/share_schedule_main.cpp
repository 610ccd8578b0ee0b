// tests/share_schedule_main.cpp — csrc/share_schedule.h behind its own main, for a build with -fsanitize=address,undefined (tests/test_share_schedule.py
// starts it as a child process; it is never loaded into Python).  stdin: one case per line,
//     qb min_rows cap mode rows  group[0] len[0] ... group[rows-1] len[rows-1]
// mode: 0 = the filling call, 1 = the sizing call (no block array), 2 = null group, 3 = null len, 4 = no row_block.  The arrays handed over are
// heap blocks of EXACTLY the sizes the contract names (cap blocks, rows entries), so that a write past them is a sanitizer report.
// stdout, per case: "n | chunks:row,row,.. ... | row_block ..." with unwritten entries printed as "-".
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "share_schedule.h"

int main() {
    unsigned qb, min_rows, cap, mode, rows;
    while (scanf("%u %u %u %u %u", &qb, &min_rows, &cap, &mode, &rows) == 5) {
        const unsigned n_in = rows > 4096 ? 4096 : rows;   // (rows outside 1..64 is a refusal the callee makes: it must not read the arrays then)
        std::vector<uint32_t> group(n_in), len(n_in);
        for (unsigned i = 0; i < n_in; ++i)
            if (scanf("%u %u", &group[i], &len[i]) != 2) return 2;
        const uint32_t UNSET = 0xDEADBEEFu;
        lh_share_block* blocks = new lh_share_block[cap];   // (cap == 0: a block of no bytes)
        for (unsigned i = 0; i < cap; ++i) { blocks[i].n = UNSET; blocks[i].chunks = UNSET; }
        uint32_t* rb = new uint32_t[n_in];
        for (unsigned i = 0; i < n_in; ++i) rb[i] = UNSET;
        const int n = lh::share_schedule(mode == 2 ? nullptr : group.data(), mode == 3 ? nullptr : len.data(), rows, qb, min_rows, mode == 1 ? nullptr : blocks, cap,
                                         mode == 4 ? nullptr : rb);
        printf("%d |", n);
        for (unsigned i = 0; i < cap; ++i) {
            if (blocks[i].n == UNSET) { printf(" -"); continue; }
            printf(" %u:", blocks[i].chunks);
            for (unsigned k = 0; k < blocks[i].n && k < 8; ++k) printf(k ? ",%u" : "%u", blocks[i].row[k]);
        }
        printf(" |");
        for (unsigned i = 0; i < n_in; ++i) { if (rb[i] == UNSET) printf(" -"); else printf(" %u", rb[i]); }
        printf("\n");
        delete[] blocks;
        delete[] rb;
    }
    return 0;
}
