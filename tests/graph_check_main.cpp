// tests/graph_check_main.cpp — csrc/graph_check.h and csrc/graph_match.h as a stand-alone program, so that the graph validator and the matcher of
// the fused plan can run under host sanitizers (tests/test_graph_check_cpu.py compiles it with -fsanitize=address,undefined and compares its
// verdicts with the library's).
//
// Input file (little endian), written by the test:
//   u32 n_graphs; per graph: u32 n_leafs, n_nodes, n_bufs, n_vals; (n_leafs + n_nodes) records of 96 bytes = struct lh_tensor whose host field
//   holds 1 + the index of the tensor's first host value (0: none); n_bufs x {u64 id, u64 nfloats, i32 dtype, i32 0}; n_vals x f32.
//   u32 n_mutations; per mutation {u32 graph, u32 tensor, u32 field, u32 0, u64 value}: one field of one tensor of a COPY of the graph is set
//   (fields: tests/graph_ops_ref.py F_*), the copy is checked and matched, one line with the return codes of lh_graph_check and lh_graph_match is
//   printed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "graph_check.h"
#include "graph_match.h"

struct GraphIn {
    uint32_t n_leafs = 0, n_nodes = 0;
    std::vector<lh_tensor> t;
    std::vector<uint64_t> host_at;   // 1 + first value, 0 = none
    std::vector<lh_buf_extent> bufs;
    std::vector<float> vals;
};

// leak checking needs ptrace, which a test's child process may not have; everything else stays on
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    static_assert(sizeof(lh_tensor) == 96, "lh_tensor layout");
    uint32_t ng = 0;
    if (!rd(f, &ng, 4)) return 2;
    std::vector<GraphIn> graphs(ng);
    for (GraphIn& g : graphs) {
        uint32_t h[4];
        if (!rd(f, h, 16)) return 2;
        g.n_leafs = h[0]; g.n_nodes = h[1];
        const size_t total = (size_t)h[0] + h[1];
        g.t.resize(total); g.host_at.resize(total);
        for (size_t i = 0; i < total; ++i) {
            unsigned char raw[96];
            if (!rd(f, raw, 96)) return 2;
            memcpy(&g.host_at[i], raw + 88, 8);
            memset(raw + 88, 0, 8);
            memcpy(&g.t[i], raw, 96);
        }
        g.bufs.resize(h[2]);
        for (lh_buf_extent& b : g.bufs) {
            struct { uint64_t id, n; int32_t dtype, pad; } e;
            if (!rd(f, &e, 24)) return 2;
            b.id = e.id; b.nfloats = e.n; b.dtype = e.dtype;
        }
        g.vals.resize(h[3]);
        if (h[3] && !rd(f, g.vals.data(), (size_t)h[3] * 4)) return 2;
    }
    uint32_t nm = 0;
    if (!rd(f, &nm, 4)) return 2;
    for (uint32_t m = 0; m < nm; ++m) {
        struct { uint32_t graph, tensor, field, pad; uint64_t value; } mu;
        if (!rd(f, &mu, 24) || mu.graph >= ng) return 2;
        const GraphIn& g = graphs[mu.graph];
        std::vector<lh_tensor> t(g.t);
        std::vector<float> vals(g.vals);            // exactly as many floats as the leafs name: a read past a leaf's values is a sanitizer report
        std::vector<std::vector<float>> own(t.size());
        for (size_t i = 0; i < t.size(); ++i) {
            if (!g.host_at[i]) continue;
            const uint64_t n = (uint64_t)g.t[i].ne[0] * g.t[i].ne[1] * g.t[i].ne[2] * g.t[i].ne[3];
            own[i].assign(vals.begin() + (g.host_at[i] - 1), vals.begin() + (g.host_at[i] - 1) + n);
            t[i].host = own[i].data();
        }
        uint32_t nl = g.n_leafs, nn = g.n_nodes;
        if (mu.field != 0 && mu.field != 16 && mu.tensor >= t.size()) return 2;
        lh_tensor* x = mu.field != 16 && mu.tensor < t.size() ? &t[mu.tensor] : nullptr;
        switch (mu.field) {
            case 0: break;
            case 1: x->op = (uint8_t)mu.value; break;
            case 2: x->src0 = (int32_t)(uint32_t)mu.value; break;
            case 3: x->src1 = (int32_t)(uint32_t)mu.value; break;
            case 4: x->storage = (int32_t)(uint32_t)mu.value; break;
            case 5: case 6: case 7: case 8: x->ne[mu.field - 5] = (uint32_t)mu.value; break;
            case 9: case 10: case 11: case 12: x->nb[mu.field - 9] = mu.value; break;
            case 13: x->view_off = mu.value; break;
            case 14: x->host = nullptr; break;
            case 15: {
                const uint32_t k = (uint32_t)(mu.value >> 32), bits = (uint32_t)mu.value;
                if (k >= own[mu.tensor].size()) return 2;
                memcpy(&own[mu.tensor][k], &bits, 4);
                break;
            }
            case 16: nl = (uint32_t)(mu.value >> 32); nn = (uint32_t)mu.value; break;
            case 17: x->flags = (uint16_t)mu.value; break;
            case 18: { const int32_t s = x->src0; x->src0 = x->src1; x->src1 = s; break; }
            default: return 2;
        }
        char msg[256];
        const int rc = lh::gc::graph_check(t.data(), nl, nn, g.bufs.data(), (uint32_t)g.bufs.size(), msg, sizeof msg);
        const int mrc = lh::gm::graph_match(t.data(), nl, nn, g.bufs.data(), (uint32_t)g.bufs.size(), nullptr);
        printf("%d %d\n", rc, mrc);
    }
    fclose(f);
    return 0;
}
