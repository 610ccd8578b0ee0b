// csrc/share_schedule.h — the block table of a tick whose pods share a prompt prefix (lh_batch_fork): a pure host function (no HIP), exported as
// lh_share_schedule and unit-tested without a GPU (tests/test_share_schedule.py, tests/share_schedule_main.cpp).  The tick executes exactly what it returns.
//
// Input: per row (= pod) the lowest pod index of its sharing group and the group's shared length, as lh_batch_share_info reports them (a pod that
// shares nothing: its own index and 0).  The rule (a FIXED function of the group state: nothing depends on timing):
//   * groups are taken in ascending order of their lowest member, members ascending;
//   * chunks = len / 128 is the number of full key chunks (ATT_TC) inside the prefix; a group with chunks == 0 or fewer than min_rows members gets no block;
//   * the members are cut into blocks of at most qb rows (2, 4 or 8), in order; a trailing block of ONE row gets no block (the row runs per-row);
//   * row_block[j] = the block that holds row j, or SHARE_NO_BLOCK.
// A block is a LIST of rows (members need not be neighbours): k_attention_split_shared reads the K / V rows of the block's first `chunks` chunks once,
// from row[0]'s cache, for all n rows.
#pragma once
#include <stdint.h>
#include "../../include/llamahip.h"

namespace lh {

constexpr uint32_t SHARE_ROWS_MAX = 64;            // rows of a batch
constexpr uint32_t SHARE_QB_MAX = 8;               // rows of a block (lh_share_block::row)
constexpr uint32_t SHARE_BLOCKS_MAX = SHARE_ROWS_MAX / 2;
constexpr uint32_t SHARE_CHUNK = 128;              // = ATT_TC (kernels_llama.h; plan.hip asserts it)
constexpr uint32_t SHARE_NO_BLOCK = 0xFFFFFFFFu;

// Returns the block count, or -1 on bad arguments: a null group / len, rows outside 1..64, qb not 2, 4 or 8, a group index that is not the lowest
// member of its group (group[j] > j, or group[group[j]] != group[j]), members of one group with different lengths, blocks given with cap below the
// count (nothing is written then).  blocks == NULL: the sizing call (cap ignored).  row_block (optional, [rows]) is written by both calls.
inline int share_schedule(const uint32_t* group, const uint32_t* len, uint32_t rows, uint32_t qb, uint32_t min_rows, lh_share_block* blocks, uint32_t cap, uint32_t* row_block) {
    if (!group || !len || rows == 0 || rows > SHARE_ROWS_MAX) return -1;
    if (qb != 2 && qb != 4 && qb != 8) return -1;
    for (uint32_t j = 0; j < rows; ++j) {
        const uint32_t g = group[j];
        if (g > j || group[g] != g || len[g] != len[j]) return -1;
    }
    lh_share_block out[SHARE_BLOCKS_MAX];
    uint32_t rb[SHARE_ROWS_MAX];
    uint32_t nb = 0;
    for (uint32_t j = 0; j < rows; ++j) rb[j] = SHARE_NO_BLOCK;
    for (uint32_t g = 0; g < rows; ++g) {   // ascending lowest member
        if (group[g] != g) continue;
        const uint32_t chunks = len[g] / SHARE_CHUNK;
        uint32_t members[SHARE_ROWS_MAX], n = 0;
        for (uint32_t j = g; j < rows; ++j) if (group[j] == g) members[n++] = j;
        if (chunks == 0 || n < min_rows) continue;
        for (uint32_t r = 0; r < n; r += qb) {
            const uint32_t take = n - r < qb ? n - r : qb;
            if (take < 2) break;   // (a trailing block of one row)
            lh_share_block& b = out[nb];
            b.n = take; b.chunks = chunks;
            for (uint32_t i = 0; i < SHARE_QB_MAX; ++i) b.row[i] = i < take ? members[r + i] : 0u;
            for (uint32_t i = 0; i < take; ++i) rb[members[r + i]] = nb;
            ++nb;
        }
    }
    if (blocks && cap < nb) return -1;
    for (uint32_t i = 0; blocks && i < nb; ++i) blocks[i] = out[i];
    for (uint32_t j = 0; row_block && j < rows; ++j) row_block[j] = rb[j];
    return (int)nb;
}

}  // namespace lh
