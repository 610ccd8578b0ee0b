// csrc/graph_check.h — what lh_graph_compute refuses before it enqueues anything: a pure host function (no HIP), exported as lh_graph_check and
// tested without a GPU (tests/test_graph_check_cpu.py; tests/graph_check_main.cpp runs the same corpora under host sanitizers).
//
// Two levels.
//   graph_check_structure  always runs, O(total), no per-op work: counts, storage owners, source indices and order, arity of the implemented
//                          ops, leafs without an op, byte strides that are whole floats, no empty extent.
//   graph_check_reach      runs in front of a node-by-node walk only: the shape rules of every op (ml.go:1711-2644), its parameter leafs, and the
//                          furthest float each kernel of kernels_generic.h touches in every operand under the addressing rule THAT kernel uses:
//                              GetRows, Mul                  rows at NE[0] pitch                (ml.go:1748, 1906)
//                              Add, Silu, Scale, SoftMax     row j of ne1*ne2*ne3 at j * ns[1]  (ml.go:2564, 2637, 2371, 2471)
//                              DiagMaskInf                   plane k of ne2*ne3 at k * ns[2]    (ml.go:2404)
//                              RMSNorm, Cpy source, MulMat, Repeat         full strides = the tensor's own span
//                              Rope                          src0's full strides on both sides          (ml.go:2274-2281)
//                          Every tensor's own span and every such reach must lie inside the owner: a registered buffer holds what the caller says
//                          (lh_buf_extent), a host leaf the nelem floats that get uploaded, any other owner its own span.
//                          Counts that run_node or a kernel keeps in 32 bits are bounded too: at most 2^31 - 1 rows for the kernels with one
//                          workgroup per row (RMSNorm, SoftMax, GetRows; MulMat: per 4 outputs), DiagMaskInf's planes and past + rows below 2^32.
// Empty tensors (an ne[k] of 0) are refused, not treated as no-ops: the span arithmetic of every level relies on ne[k] - 1.
// All offsets are computed in 128 bits: ne < 2^32 and nb / 4 < 2^62, so no sum of four products can wrap.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/llamahip.h"

namespace lh {
namespace gc {

typedef unsigned __int128 u128;

enum { NONE = 0, ADD = 2, MUL = 4, REPEAT = 10, SILU = 17, RMS_NORM = 19, MUL_MAT = 20, SCALE = 21, CPY = 22, RESHAPE = 23, VIEW = 24, PERMUTE = 25,
       GET_ROWS = 27, DIAG_MASK_INF = 28, SOFT_MAX = 29, ROPE = 30 };

constexpr uint64_t MAX_OWNER_FLOATS = 1ull << 40;   // 4 TiB of scratch per graph: beyond any device, and the arena's byte count stays far inside 64 bits
constexpr uint64_t MAX_ROPE_POSITIONS = 1u << 20;   // the cos/sin table is built on the host per position (ensure_rope_table)
constexpr uint64_t MAX_GRID = 0x7fffffffull;        // workgroups of one launch: kernels with one workgroup per row (or per 4 outputs) take no more rows

inline int fail(char* msg, uint64_t cap, int code, const char* fmt, ...) __attribute__((format(printf, 4, 5)));
inline int fail(char* msg, uint64_t cap, int code, const char* fmt, ...) {
    if (msg && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, (size_t)cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

// sources an implemented op dereferences: 0 (a view / leaf: nothing runs), 1 (src0), 2 (src0 and src1); 255 = not implemented
inline uint8_t arity(uint8_t op) {
    switch (op) {
        case NONE: case RESHAPE: case VIEW: case PERMUTE: return 0;
        case RMS_NORM: case REPEAT: case SILU: case CPY: case SOFT_MAX: return 1;
        case GET_ROWS: case MUL: case ADD: case SCALE: case DIAG_MASK_INF: case ROPE: case MUL_MAT: return 2;
        default: return 255;
    }
}

inline int graph_check_structure(const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, char* msg, uint64_t cap) {
    if (!T && (n_leafs || n_nodes)) return fail(msg, cap, LH_EINVAL, "no tensor array");
    if ((uint64_t)n_leafs + n_nodes > 0x7fffffffull) return fail(msg, cap, LH_EINVAL, "%u leafs + %u nodes: more than int32 indices can name", n_leafs, n_nodes);
    const uint32_t total = n_leafs + n_nodes;
    const int32_t tot = (int32_t)total;
    for (uint32_t i = 0; i < total; ++i) {
        const lh_tensor& t = T[i];
        if (t.storage < 0 || t.storage >= tot) return fail(msg, cap, LH_EINVAL, "tensor %u: storage index %d out of range", i, t.storage);
        if (t.src0 < -1 || t.src0 >= tot || t.src1 < -1 || t.src1 >= tot) return fail(msg, cap, LH_EINVAL, "tensor %u: source index out of range", i);
        if (T[t.storage].storage != t.storage) return fail(msg, cap, LH_EINVAL, "tensor %u: storage owner %d is itself a view", i, t.storage);
        if ((t.nb[0] | t.nb[1] | t.nb[2] | t.nb[3]) & 3) return fail(msg, cap, LH_ESHAPE, "tensor %u: a byte stride is not a multiple of 4", i);
        if (!t.ne[0] || !t.ne[1] || !t.ne[2] || !t.ne[3]) return fail(msg, cap, LH_ESHAPE, "tensor %u: an extent of 0 elements", i);
        if (i < n_leafs) {
            if (t.op != NONE) return fail(msg, cap, LH_EINVAL, "tensor %u: a leaf with op %d", i, (int)t.op);
            continue;
        }
        // nodes come after their node sources (post-order, ml.go:647-697); leaf sources may stand anywhere
        if ((t.src0 >= (int32_t)i && (uint32_t)t.src0 >= n_leafs) || (t.src1 >= (int32_t)i && (uint32_t)t.src1 >= n_leafs))
            return fail(msg, cap, LH_EINVAL, "node %u is listed before one of its sources", i);
        const uint8_t ar = arity(t.op);
        if (ar == 255) return fail(msg, cap, LH_EUNSUPPORTED, "[HALT] Please implement : op %d (the reference halts on it too, ml.go:1536-1700) at tensor %u", (int)t.op, i);
        if ((ar >= 1 && t.src0 < 0) || (ar >= 2 && t.src1 < 0)) return fail(msg, cap, LH_EINVAL, "tensor %u: op %d lacks a source", i, (int)t.op);
    }
    return LH_OK;
}

inline u128 nelem(const lh_tensor& t) { return (u128)t.ne[0] * t.ne[1] * t.ne[2] * t.ne[3]; }
inline u128 rows(const lh_tensor& t) { return (u128)t.ne[1] * t.ne[2] * t.ne[3]; }
inline u128 span(const lh_tensor& t) {   // furthest float through the tensor's own strides, + 1
    u128 e = 1;
    for (int k = 0; k < 4; ++k) e += (u128)(t.ne[k] - 1) * (t.nb[k] / 4);
    return e;
}
inline bool contiguous(const lh_tensor& t) {   // ml.go:206-211
    return t.nb[0] == 4 && t.nb[1] == t.nb[0] * t.ne[0] && t.nb[2] == t.nb[1] * t.ne[1] && t.nb[3] == t.nb[2] * t.ne[2];
}
inline bool same_shape(const lh_tensor& a, const lh_tensor& b) { return a.ne[0] == b.ne[0] && a.ne[1] == b.ne[1] && a.ne[2] == b.ne[2] && a.ne[3] == b.ne[3]; }
inline u128 flat_rows(const lh_tensor& x, u128 nrows, uint32_t nc) { return (nrows - 1) * (x.nb[1] / 4) + nc; }   // row j at j * ns[1]
// a host-readable parameter leaf: an owner leaf without a buffer whose host pointer the call may read
inline const float* host_values(const lh_tensor* T, int32_t j) {
    const lh_tensor& b = T[j];
    return (b.op == NONE && b.storage == j && !b.buf) ? b.host : nullptr;
}
inline bool castable_u32(float v) { return v >= 0.f && v < 4294967296.f; }   // false for NaN

// out_size (optional): floats every owner holds, by tensor index (0 for tensors that are views)
inline int graph_check_reach(const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, char* msg, uint64_t cap,
                             std::vector<uint64_t>* out_size = nullptr) {
    const uint32_t total = n_leafs + n_nodes;
    std::vector<uint64_t> size(total, 0);
    u128 scratch = 0;
    std::vector<int8_t> q8(total, 0);   // owner is a registered buffer of another dtype than f32: that dtype (1 = f16, 2 = block-int4, 7 = block-int8)
    std::vector<const lh_buf_extent*> sorted;
    for (uint32_t k = 0; k < n_bufs; ++k) sorted.push_back(bufs + k);
    std::sort(sorted.begin(), sorted.end(), [](const lh_buf_extent* a, const lh_buf_extent* b) { return a->id < b->id; });
    for (uint32_t i = 0; i < total; ++i) {
        const lh_tensor& t = T[i];
        if ((uint32_t)t.storage != i) continue;
        if (t.buf) {
            auto it = std::lower_bound(sorted.begin(), sorted.end(), t.buf, [](const lh_buf_extent* a, lh_buf id) { return a->id < id; });
            if (it == sorted.end() || (*it)->id != t.buf) return fail(msg, cap, LH_EINVAL, "tensor %u: unknown buffer %llu", i, (unsigned long long)t.buf);
            size[i] = (*it)->nfloats;
            q8[i] = (int8_t)(*it)->dtype;
            continue;
        }
        const u128 s = t.host ? nelem(t) : span(t);   // host data is uploaded flat, nelem floats
        scratch += s;
        if (s > MAX_OWNER_FLOATS || scratch > MAX_OWNER_FLOATS) return fail(msg, cap, LH_ENOMEM, "tensor %u: the graph's scratch tensors hold more than 2^40 floats", i);
        size[i] = (uint64_t)s;
    }
    // every tensor lies inside its owner (a Go slice that did not would have panicked when the view was made)
    for (uint32_t i = 0; i < total; ++i) {
        const lh_tensor& t = T[i];
        const u128 e = (u128)t.view_off + span(t);
        if (e > size[t.storage])
            return fail(msg, cap, LH_ESHAPE, "tensor %u: views reach %llu floats, buffer holds %llu", i, (unsigned long long)std::min<u128>(e, ~0ull), (unsigned long long)size[t.storage]);
    }
    // inside(x, n): the first n floats from x's base lie inside x's owner
    auto inside = [&](int32_t j, u128 n) { return (u128)T[j].view_off + n <= size[T[j].storage]; };
#define GC_REACH(j, n) do { if (!inside((j), (n))) return fail(msg, cap, LH_ESHAPE, "tensor %u: op %d reaches past the storage of tensor %d", i, (int)t.op, (int)(j)); } while (0)
#define GC_SHAPE(cond, text) do { if (!(cond)) return fail(msg, cap, LH_ESHAPE, "tensor %u: " text, i); } while (0)
#define GC_LAUNCH(cond, text) do { if (!(cond)) return fail(msg, cap, LH_EUNSUPPORTED, "tensor %u: " text, i); } while (0)   // a 32-bit count of run_node / its kernel
    for (uint32_t i = n_leafs; i < total; ++i) {
        const lh_tensor& t = T[i];
        if (arity(t.op) == 0) continue;
        const int32_t ia = t.src0, ib = arity(t.op) == 2 ? t.src1 : -1, id = (int32_t)i;
        const lh_tensor& a = T[ia];
        if (q8[a.storage] || q8[t.storage] || (ib >= 0 && q8[T[ib].storage])) {
            const bool f16 = q8[a.storage] == 1 || q8[t.storage] == 1 || (ib >= 0 && q8[T[ib].storage] == 1);
            const bool q4 = q8[a.storage] == 2 || q8[t.storage] == 2 || (ib >= 0 && q8[T[ib].storage] == 2);
            return fail(msg, cap, LH_EUNSUPPORTED, "tensor %u: %s weights are only supported inside the fused LLaMA plan", i, f16 ? "f16" : q4 ? "block-int4" : "block-int8");
        }
        switch (t.op) {
            case GET_ROWS: {   // ml.go:1711-1750
                const lh_tensor& b = T[ib];
                if (t.ne[0] != a.ne[0] || (u128)t.ne[1] != nelem(b) || a.nb[0] != 4)
                    return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT]ComputeForwardGetRows : wrong dimensions!", i);
                const float* ids = host_values(T, ib);
                if (!ids) return fail(msg, cap, LH_EUNSUPPORTED, "tensor %u: GetRows: indices must be a host leaf (they cannot be bounds-checked on the device)", i);
                uint32_t top = 0;
                for (uint32_t k = 0; k < t.ne[1]; ++k) {
                    if (!castable_u32(ids[k]) || (uint32_t)ids[k] >= a.ne[1])
                        return fail(msg, cap, LH_EINVAL, "tensor %u: GetRows: row index %g outside the table of %u rows", i, (double)ids[k], a.ne[1]);
                    top = std::max(top, (uint32_t)ids[k]);
                }
                GC_LAUNCH(t.ne[1] <= MAX_GRID, "GetRows: more than 2^31 - 1 rows in one launch");
                GC_REACH(ia, ((u128)top + 1) * a.ne[0]);
                GC_REACH(id, (u128)t.ne[1] * t.ne[0]);
                break;
            }
            case RMS_NORM:   // ml.go:1753-1812; rows through all strides, elements of a row adjacent
                GC_SHAPE(same_shape(a, t), "RMSNorm: [dst] and [src0] have different shapes");
                GC_SHAPE(a.nb[0] == 4 && t.nb[0] == 4, "RMSNorm: rows must be contiguous (ml.go:1756)");
                GC_LAUNCH(rows(a) <= MAX_GRID, "RMSNorm: more than 2^31 - 1 rows in one launch");
                break;
            case REPEAT:     // ml.go:1822-1868
                GC_SHAPE(a.ne[2] == 1 && a.ne[3] == 1 && t.ne[2] == 1 && t.ne[3] == 1, "Repeat: only 2-D tensors (ml.go:1831-1835)");
                GC_SHAPE(t.ne[0] % a.ne[0] == 0 && t.ne[1] % a.ne[1] == 0, "Repeat: [dst] is no multiple of [src0] (ml.go:1825)");
                GC_SHAPE(a.nb[0] == 4 && t.nb[0] == 4, "Repeat: rows must be contiguous (ml.go:1845-1846)");
                break;
            case MUL: {      // ml.go:1877-1914: every row at NE[0] pitch, i.e. flat
                const lh_tensor& b = T[ib];
                if (!same_shape(a, b) || !same_shape(a, t)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardMulFP32 : different shapes!", i);
                GC_REACH(ia, nelem(a)); GC_REACH(ib, nelem(a)); GC_REACH(id, nelem(a));
                break;
            }
            case ADD: {      // ml.go:2515-2584
                const lh_tensor& b = T[ib];
                if (b.nb[0] != 4) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardAddFP32 : [src1] is NOT contiguous!", i);
                GC_SHAPE(same_shape(a, b) && same_shape(a, t), "Add: different shapes (ml.go:2517)");
                GC_SHAPE(a.nb[0] == 4 && t.nb[0] == 4, "Add: rows must be contiguous (ml.go:2543-2544)");
                GC_REACH(ia, flat_rows(a, rows(a), a.ne[0])); GC_REACH(ib, flat_rows(b, rows(a), a.ne[0])); GC_REACH(id, flat_rows(t, rows(a), a.ne[0]));
                break;
            }
            case SILU:
                if (!contiguous(a)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardSiluFP32 : [src0] is NOT contiguous!", i);
                if (!contiguous(t)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardSiluFP32 : [dst] is NOT contiguous!", i);
                GC_SHAPE(same_shape(a, t), "Silu: different shapes (ml.go:2603)");
                break;
            case SCALE: {    // ml.go:2331-2374, in place
                if (!contiguous(a)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardScaleFP32 : [src0] is NOT contiguous!", i);
                if (!contiguous(t)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardScaleFP32 : [dst] is NOT contiguous!", i);
                GC_SHAPE(same_shape(a, t), "Scale: different shapes (ml.go:2335)");
                GC_SHAPE(nelem(T[ib]) == 1, "Scale: the factor is not a scalar (ml.go:2336)");
                break;
            }
            case CPY:        // ml.go:2110-2240
                if (!contiguous(t)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardDupFP32 : [dst] is NOT contiguous!", i);
                if (nelem(t) != nelem(a)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardDupFP32 : [dst] and [src0] capacities are different!", i);
                break;
            case DIAG_MASK_INF: {   // ml.go:2377-2414, in place: plane k of ne2 * ne3 at k * ns[2]
                GC_SHAPE(same_shape(a, t), "DiagMaskInf: different shapes");
                GC_SHAPE(nelem(T[ib]) == 1, "DiagMaskInf: src1 is not one value (ml.go:2381)");
                const float* p = host_values(T, ib);
                GC_SHAPE(p != nullptr, "DiagMaskInf: `past` must be a host leaf");
                if (!castable_u32(p[0])) return fail(msg, cap, LH_EINVAL, "tensor %u: DiagMaskInf: past %g is no uint32", i, (double)p[0]);
                // g_diag_mask_inf counts planes and computes past + j in 32 bits
                GC_LAUNCH((uint64_t)t.ne[2] * t.ne[3] <= 0xffffffffull, "DiagMaskInf: 2^32 planes or more");
                GC_LAUNCH((uint64_t)(uint32_t)p[0] + t.ne[1] <= 0x100000000ull, "DiagMaskInf: past + rows wraps in 32 bits");
                GC_REACH(id, ((u128)t.ne[2] * t.ne[3] - 1) * (t.nb[2] / 4) + (u128)(t.ne[1] - 1) * (t.nb[1] / 4) + (u128)(t.ne[0] - 1) * (t.nb[0] / 4) + 1);
                break;
            }
            case SOFT_MAX:   // ml.go:2432-2505, in place
                if (!contiguous(a)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardSoftMaxFP32 : [src0] is NOT contiguous!", i);
                if (!contiguous(t)) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardSoftMaxFP32 : [dst] is NOT contiguous!", i);
                GC_SHAPE(same_shape(a, t), "SoftMax: different shapes (ml.go:2436)");
                GC_LAUNCH(rows(t) <= MAX_GRID, "SoftMax: more than 2^31 - 1 rows in one launch");
                break;
            case ROPE: {     // ml.go:2253-2328, in place on adjacent pairs.  src0's NE and NB address both sides (ml.go:2274-2281); [dst] is a ViewTensor of
                             // src0 (ml.go:1016): the same Data under strides of its own - packed ones, when src0 is a permuted view - which nothing reads
                const lh_tensor& b = T[ib];
                const float* p = host_values(T, ib);
                if (nelem(b) != 3 || !p) return fail(msg, cap, LH_ESHAPE, "tensor %u: [HALT] ComputeForwardRopeFP32 : src1 has NOT EXACT 3 elements!", i);
                if (!castable_u32(p[0]) || !castable_u32(p[1]) || !castable_u32(p[2]))
                    return fail(msg, cap, LH_EINVAL, "tensor %u: Rope: parameters (%g, %g, %g) are no uint32", i, (double)p[0], (double)p[1], (double)p[2]);
                const uint32_t past = (uint32_t)p[0], dims = (uint32_t)p[1], mode = (uint32_t)p[2];
                if (dims == 0 || dims % 2 || dims > a.ne[0]) return fail(msg, cap, LH_ESHAPE, "tensor %u: Rope: dims %u not supported", i, dims);
                GC_SHAPE(a.nb[0] == 4, "Rope: pairs must be adjacent (ml.go:2282)");
                GC_SHAPE(same_shape(a, t) && a.storage == t.storage && a.view_off == t.view_off, "Rope: [dst] is not the view of [src0] it rotates in place (ml.go:1016)");
                if ((uint64_t)past + a.ne[2] > 0xffffffffull) return fail(msg, cap, LH_EINVAL, "tensor %u: Rope: past %u + %u positions wraps", i, past, a.ne[2]);
                if ((uint64_t)(mode == 0 ? past : 0) + a.ne[2] > MAX_ROPE_POSITIONS)
                    return fail(msg, cap, LH_EUNSUPPORTED, "tensor %u: Rope: position %llu beyond the %llu the cos/sin table is built for", i,
                                (unsigned long long)((mode == 0 ? past : 0) + (uint64_t)a.ne[2]), (unsigned long long)MAX_ROPE_POSITIONS);
                break;
            }
            case MUL_MAT: {  // ml.go:1976-2098
                const lh_tensor& b = T[ib];
                if (a.ne[0] != b.ne[0] || a.ne[2] != b.ne[2] || a.ne[3] != b.ne[3]) return fail(msg, cap, LH_ESHAPE, "tensor %u: MulMat: incompatible shapes (ml.go:290-292)", i);
                if (a.nb[0] != 4 || b.nb[0] != 4) return fail(msg, cap, LH_ESHAPE, "tensor %u: MulMat: operands must be contiguous along K (ml.go:1950, 1967)", i);
                if (a.dtype != 0) return fail(msg, cap, LH_EUNSUPPORTED, "tensor %u: MulMat: %s weights are only supported inside the fused LLaMA plan", i, a.dtype == 1 ? "f16" : a.dtype == 2 ? "block-int4" : "block-int8");
                GC_SHAPE(t.ne[0] == a.ne[1] && t.ne[1] == b.ne[1] && t.ne[2] == a.ne[2] && t.ne[3] == a.ne[3], "MulMat: [dst] is not (src0.ne1, src1.ne1, src0.ne2, src0.ne3) (ml.go:295-318)");
                GC_LAUNCH((rows(a) * b.ne[1] + 3) / 4 <= MAX_GRID, "MulMat: more than 2^33 - 4 outputs in one launch");   // g_mul_mat: one wave per output, four per workgroup
                break;
            }
            default: break;
        }
    }
#undef GC_REACH
#undef GC_SHAPE
#undef GC_LAUNCH
    if (out_size) out_size->swap(size);
    return LH_OK;
}

inline int graph_check(const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, char* msg, uint64_t cap) {
    if (msg && cap) msg[0] = 0;
    if (n_bufs && !bufs) return fail(msg, cap, LH_EINVAL, "no buffer extents");
    const int rc = graph_check_structure(T, n_leafs, n_nodes, msg, cap);
    return rc ? rc : graph_check_reach(T, n_leafs, n_nodes, bufs, n_bufs, msg, cap);
}

}  // namespace gc
}  // namespace lh
