// csrc/feed_schedule.h — the pass schedule of lh_batch_feed: a pure host function (no HIP), exported as lh_feed_schedule and unit-tested
// without a GPU (tests/test_feed_schedule.py).  lh_batch_feed executes exactly what it returns.
//
// The rule (a FIXED partition of the fed rows: nothing depends on timing):
//   * a pod with n_tokens >= solo_min is a SOLO pass: one Eval on the pod's own plan (tile GEMM, two-pass stream routes, flash attention);
//   * all other fed rows are concatenated in pod order, positions ascending, and cut into BATCHED passes of at most 64 rows.  A pod's rows in one
//     pass are a segment {pod, row0, n, pos0}; a segment may continue in the next pass (which then sees the earlier pass's keys in the pod's cache);
//   * a pass of one row, and every segment of a pass whose row count the caller's `sizes_ok` mask refuses (bit n - 1: n rows of different streams may
//     share one weight pass on this plan), runs as a solo pass of that segment - same results, more weight passes;
//   * the attention of a batched pass works on query blocks: at most qb consecutive rows of ONE segment; a block never crosses a segment or a pass.
// Order of the passes: the batched partition first (pod order), then the solo pods in pod order.  Pods own their caches, so the order between
// passes of different pods changes no result; passes of one pod are in ascending position.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/llamahip.h"

namespace lh {

constexpr uint32_t FEED_PASS_ROWS = 64;

struct FeedSchedule {
    std::vector<lh_feed_pass> passes;
    std::vector<lh_feed_seg> segs;
    std::vector<lh_feed_block> blocks;
};

inline void feed_schedule(const uint32_t* n_tokens, const uint32_t* past, uint32_t rows, uint32_t solo_min, uint32_t qb, uint64_t sizes_ok, FeedSchedule* out) {
    out->passes.clear(); out->segs.clear(); out->blocks.clear();
    if (qb == 0) qb = 1;
    if (solo_min == 0) solo_min = 1;
    auto solo_pass = [&](uint32_t pod, uint32_t n, uint32_t pos0) {
        out->passes.push_back(lh_feed_pass{LH_FEED_SOLO, (uint32_t)out->segs.size(), 1u, (uint32_t)out->blocks.size(), 0u, n});
        out->segs.push_back(lh_feed_seg{pod, 0u, n, pos0});
    };
    // the batched partition: walk the rows of the pods below solo_min and close a pass at 64 rows
    std::vector<lh_feed_seg> cur;
    uint32_t cur_rows = 0;
    auto close = [&]() {
        if (!cur_rows) return;
        const bool batched = cur_rows >= 2 && ((sizes_ok >> (cur_rows - 1)) & 1u);
        if (!batched) {
            for (const lh_feed_seg& s : cur) solo_pass(s.pod, s.n, s.pos0);
        } else {
            lh_feed_pass p = {LH_FEED_BATCHED, (uint32_t)out->segs.size(), (uint32_t)cur.size(), (uint32_t)out->blocks.size(), 0u, cur_rows};
            for (const lh_feed_seg& s : cur) {
                out->segs.push_back(s);
                for (uint32_t r = 0; r < s.n; r += qb) out->blocks.push_back(lh_feed_block{s.row0 + r, s.n - r < qb ? s.n - r : qb});
            }
            p.nblk = (uint32_t)out->blocks.size() - p.blk0;
            out->passes.push_back(p);
        }
        cur.clear(); cur_rows = 0;
    };
    for (uint32_t i = 0; i < rows; ++i) {
        if (!n_tokens[i] || n_tokens[i] >= solo_min) continue;
        uint32_t done = 0;
        while (done < n_tokens[i]) {
            const uint32_t take = n_tokens[i] - done < FEED_PASS_ROWS - cur_rows ? n_tokens[i] - done : FEED_PASS_ROWS - cur_rows;
            cur.push_back(lh_feed_seg{i, cur_rows, take, past[i] + done});
            cur_rows += take; done += take;
            if (cur_rows == FEED_PASS_ROWS) close();
        }
    }
    close();
    for (uint32_t i = 0; i < rows; ++i)
        if (n_tokens[i] && n_tokens[i] >= solo_min) solo_pass(i, n_tokens[i], past[i]);
}

}  // namespace lh
