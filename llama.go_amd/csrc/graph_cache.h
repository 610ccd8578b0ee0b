// csrc/graph_cache.h — the one holder of a captured hipGraph and the one rule that keeps it fresh:
//
//   whoever re-allocates something a captured launch holds bumps its generation; every graph compares its key where it is used.
//
// A key is a plain struct of everything the captured launches hold by value: addresses the caller passes in, generation counters of buffers that
// grow (Plan::scratch_gen / out_gen / smp_gen, lh_ctx::splitk_gen, Batch::smp_gen), switches that choose a kernel.  Keys are compared with memcmp,
// so a key must have no padding (flags are uint32_t / uint64_t, never bool); a key that has some does not compile.
#pragma once
#include "common.h"

#include <cstring>
#include <type_traits>

namespace lh {

template <typename Key>
struct CapturedGraph {
    static_assert(std::has_unique_object_representations_v<Key>, "a graph key is compared with memcmp: no padding, no bool, no float");
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    Key key = {};        // what exec was captured for
    uint64_t warm = 0;   // bit i: the shape the owner numbers i has run eagerly (an eager run sets kernel attributes and allocates, a capture must not)

    void drop() {
        if (exec) { hipGraphExecDestroy(exec); exec = nullptr; }
        if (graph) { hipGraphDestroy(graph); graph = nullptr; }
    }
    // drops a graph captured for another key; true: an exec for k is left
    bool current(const Key& k) {
        if (exec && memcmp(&key, &k, sizeof k)) drop();
        return exec != nullptr;
    }
    // captures what enqueue() puts on ctx->stream (int(): 0 or an LH_E* code) and instantiates it for key k
    template <typename F>
    int capture(lh_ctx* ctx, const Key& k, const char* what, F&& enqueue) {
        drop();
        // Relaxed: other pods' threads keep allocating / copying while this one captures (server.go:88-101 runs pods concurrently).  The
        // captured stream is non-blocking and nothing inside the capture touches the legacy stream; in the stricter modes a
        // synchronous hipMemcpy of ANOTHER thread invalidated this capture (tests/test_gpu_llama.py::test_concurrent_pods_share_one_model).
        LH_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
        const int rc = enqueue();
        // (the capture is ended whatever enqueue() returned; its error counts only where enqueue() had none)
        if (const hipError_t e = hipStreamEndCapture(ctx->stream, &graph); !rc && e != hipSuccess) LH_FAIL(ctx, LH_EHIP, "hipStreamEndCapture%s: %s", what, hipGetErrorString(e));
        if (rc) { drop(); return rc; }   // the half-made graph
        LH_HIP(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        key = k;
        return 0;
    }
    int launch(lh_ctx* ctx) {
        LH_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
        return 0;
    }
    // One use of a graph whose launches may also run eagerly: the first use of a shape (warm_bit) and every use with use_graph off enqueue
    // eagerly; every other one replays the graph, captured anew when the key has changed.
    template <typename F>
    int run(lh_ctx* ctx, bool use_graph, uint32_t warm_bit, const Key& k, const char* what, F&& enqueue) {
        const uint64_t bit = 1ull << warm_bit;
        if (!use_graph || !(warm & bit)) {
            warm |= bit;
            return enqueue();
        }
        if (!current(k)) {
            if (const int rc = capture(ctx, k, what, enqueue)) return rc;
        }
        return launch(ctx);
    }
};

// the five decode slots of a Plan (plan.h): generations of the scratch, of the output list (slots that advance) and of the sampler (slots that sample)
struct DecodeKey {
    uint64_t scratch_gen, out_gen, smp_gen;
};

}  // namespace lh
