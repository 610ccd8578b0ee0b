// csrc/graph_match.h — the gate of lh_graph_compute: does this array describe the graph llama.Eval builds (pkg/llama/llama.go:211-389)?  A pure
// host function (no HIP), used by lh_graph_compute (csrc/graph.hip) and exported as lh_graph_match; tested without a GPU
// (tests/test_graph_match_cpu.py; tests/graph_check_main.cpp runs the same corpora under host sanitizers).
//
// The rule.  A graph that is accepted runs as the fused plan, whose result is a function of MatchInfo (geometry, N, past, the leaf of every
// weight, the two cache owners, the token ids) and of the data alone.  So a graph may be accepted only if the reference's sequential walk of it
// (ml.go:1501-1526) computes exactly that function, and every node the pattern claims is therefore verified in full against what the pattern
// implies, not by its op alone:
//   - a compute result (GetRows, RMSNorm, Repeat, Mul, MulMat, Silu, Add) owns storage of its own: storage == its index, view_off 0, no buffer;
//     shape exact in all four extents, byte strides packed in all four - those of unit extents too: the row rules of Add / Silu / Scale / SoftMax
//     step at ns[1] over ne1 * ne2 * ne3 rows whatever ne[1] is, and `contiguous` (ml.go:206-211) reads all four;
//   - a view (View1D, Reshape3D, Permute) and an in-place op (Rope, Scale, DiagMaskInf, SoftMax) lies at its source's owner and offset, with the
//     one shape and the strides the reference's constructor gives it;
//   - a Cpy lies at its destination: a scratch leaf of its own (packed, used once) or the View1D of a cache slot;
//   - the K / V stores of a layer stand in front of the first node that reads what they write (the K Rope, the V^T copy);
//   - weight leafs are owners of registered buffers, packed, at offset 0, inside the buffer; parameter leafs are host-readable owners of exactly
//     the values the op reads, and every value is castable_u32 before it is cast;
//   - counts stay inside what graph_check_reach accepts (rope positions, outputs of one MulMat launch, scratch floats per graph).
// Together these imply graph_check_reach for an f32 graph: an accepted graph is one the node path would run too (block-int8, block-int4 and f16 weights are exempt
// from its dtype rule only - the node path has no kernel for them).  Anything else is not an error: the graph runs node by node.
//
// The device is behind `Lookup`: bool lookup(lh_buf id, BufInfo* out).  lh_graph_compute answers from its buffer table; lh_graph_match from the
// lh_buf_extent array lh_graph_check takes.  An extent knows no rows / cols: for a block-int8 buffer the device-free entry requires
// nfloats == ne0 * ne1 where the device one compares rows and cols.
#pragma once
#include "graph_check.h"

namespace lh {
namespace gm {

struct BufInfo {
    uint64_t nfloats = 0;
    int dtype = 0;
    uint32_t rows = 0, cols = 0;
    bool has_shape = false;   // rows / cols are known (block-int8 buffers of a device)
};

// order of MatchInfo::weights within a layer; after the layers: tok_embeddings, norm, output
enum { W_ATTN_NORM = 0, W_WQ, W_WK, W_WV, W_WO, W_FFN_NORM, W_W1, W_W2, W_W3, W_PER_LAYER, W_TOK_EMB = 0, W_NORM, W_OUTPUT, W_TAIL };

struct MatchInfo {
    uint32_t N = 0, past = 0, V = 0, d = 0, H = 0, hd = 0, L = 0, F = 0, ctx = 0;
    int wtype = 0;
    int kc_owner = -1, vc_owner = -1, tokens_leaf = -1;
    int emb_node = -1;                // `embeddings` of llama.Eval (llama.go:381): the final norm * weight rows, source of the lm_head
    std::vector<int32_t> weights;     // leaf index of every weight: W_PER_LAYER per layer, then W_TAIL
    std::vector<uint32_t> tokens;
};

constexpr uint64_t MAX_CACHE_FLOATS = 1ull << 40;

template <class Lookup>
struct Matcher {
    const lh_tensor* T;
    uint32_t total, n_leafs;
    Lookup lookup;
    MatchInfo mi;
    Matcher(const lh_tensor* t, uint32_t n_leafs_, uint32_t n_nodes, Lookup l) : T(t), total(n_leafs_ + n_nodes), n_leafs(n_leafs_), lookup(l) {}

    // Every node the pattern walks over is marked; the match only holds if ALL nodes of the graph were claimed (extra outputs or
    // side-effect copies expanded into the same graph would otherwise be silently skipped by the fused plan).  Leafs: 1 = the destination
    // of a Cpy (used once), 2 = a parameter leaf.
    mutable std::vector<uint8_t> claimed;
    struct Store { uint64_t off; uint32_t cpy; };
    std::vector<Store> stores;   // Cpy nodes into a View of a registered buffer, in graph order
    int wtype_seen = -1;
    mutable uint64_t scratch = 0;

    bool is(int i, int op) const {
        if (i < 0 || (uint32_t)i >= total || T[i].op != op) return false;
        claimed[i] = 1;
        return true;
    }
    int s0(int i) const { return T[i].src0; }
    int s1(int i) const { return T[i].src1; }
    bool scratch_add(uint64_t n) const {   // graph_check_reach: no scratch owner and no graph holds more than MAX_OWNER_FLOATS
        if (n > gc::MAX_OWNER_FLOATS) return false;
        scratch += n;
        return scratch <= gc::MAX_OWNER_FLOATS;
    }
    // shape + byte strides, all four
    bool shaped(int i, uint64_t n0, uint64_t n1, uint64_t n2, uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3) const {
        const lh_tensor& t = T[i];
        return t.ne[0] == n0 && t.ne[1] == n1 && t.ne[2] == n2 && t.ne[3] == 1 && t.nb[0] == b0 && t.nb[1] == b1 && t.nb[2] == b2 && t.nb[3] == b3;
    }
    bool packed(int i, uint64_t n0, uint64_t n1, uint64_t n2) const { return shaped(i, n0, n1, n2, 4, 4 * n0, 4 * n0 * n1, 4 * n0 * n1 * n2); }
    bool at(int i, int owner, uint64_t off) const { return T[i].storage == owner && T[i].view_off == off; }
    bool alias(int i, int j) const { return at(i, T[j].storage, T[j].view_off); }
    // a compute result: claimed, packed [n0, n1, n2], storage of its own
    bool fresh(int i, int op, uint64_t n0, uint64_t n1, uint64_t n2) const {
        if (!is(i, op) || !packed(i, n0, n1, n2) || !at(i, i, 0) || T[i].buf) return false;
        if (op == gc::MUL_MAT && (n0 * n1 * n2 + 3) / 4 > gc::MAX_GRID) return false;   // g_mul_mat: one wave per output, four per workgroup
        return scratch_add(n0 * n1 * n2);
    }
    // Cpy(src, new tensor): the destination is a scratch leaf of this shape that nothing else is copied into
    bool cpy_into_leaf(int i, uint64_t n0, uint64_t n1, uint64_t n2) const {
        if (!is(i, gc::CPY)) return false;
        const int dst = s1(i);
        if (dst < 0 || (uint32_t)dst >= n_leafs || claimed[dst]) return false;
        const lh_tensor& t = T[dst];
        if (t.op != gc::NONE || t.buf || !at(dst, dst, 0) || !packed(dst, n0, n1, n2) || !packed(i, n0, n1, n2) || !at(i, dst, 0)) return false;
        claimed[dst] = 1;
        return scratch_add(n0 * n1 * n2);
    }
    // persistent weight leaf of the expected shape.  Matrices may be f32, f16, block-int4 or block-int8 (all the same dtype within a model); norm vectors and
    // the embedding table are always f32.  (Strides count fp32-sized logical elements for every dtype, as they do for block-int8.)
    bool weight(int i, uint32_t ne0, uint32_t ne1, bool matrix, int32_t* slot) {
        if (i < 0 || (uint32_t)i >= n_leafs) return false;
        const lh_tensor& t = T[i];
        if (t.op != gc::NONE || !t.buf || !at(i, i, 0) || !packed(i, ne0, ne1, 1)) return false;
        BufInfo b;
        if (!lookup(t.buf, &b) || b.nfloats < (uint64_t)ne0 * ne1 || b.dtype != (int)t.dtype) return false;
        if (b.dtype != 0 && !(matrix && (b.dtype == 7 || b.dtype == 2 || b.dtype == 1))) return false;
        if ((b.dtype == 7 || b.dtype == 2) && (b.has_shape ? (b.rows != ne1 || b.cols != ne0) : b.nfloats != (uint64_t)ne0 * ne1)) return false;
        if (matrix) {
            if (wtype_seen < 0) wtype_seen = b.dtype;
            else if (wtype_seen != b.dtype) return false;
        }
        *slot = i;
        return true;
    }
    // h = Mul(Repeat(gamma, r), r = RMSNorm(x)), all [d, N]  ->  x.  For N = 1 ml.Repeat hands gamma itself back (equal shapes, ml.go:487-513) and
    // Mul reads the leaf; for any other N a Mul over the [d, 1] leaf breaks Mul's shape rule
    bool norm_mul(int h, int* x, int32_t* slot) {
        const uint32_t d = mi.d, n = mi.N;
        if (!fresh(h, gc::MUL, d, n, 1)) return false;
        int g = s0(h);
        const int r = s1(h);
        if (!fresh(r, gc::RMS_NORM, d, n, 1)) return false;
        if (!(n == 1 && g >= 0 && (uint32_t)g < n_leafs)) {
            if (!fresh(g, gc::REPEAT, d, n, 1)) return false;
            g = s0(g);
        }
        if (!weight(g, d, 1, false, slot)) return false;
        *x = s0(r);
        return true;
    }
    // an owner leaf whose n host values the call may read (graph_check.h host_values), exactly n of them
    const float* host_param(int i, uint32_t n) const {
        if (i < 0 || (uint32_t)i >= n_leafs || claimed[i] == 1) return nullptr;
        const lh_tensor& t = T[i];
        if (t.op != gc::NONE || t.buf || !t.host || !at(i, i, 0)) return nullptr;
        if (t.ne[0] != n || t.ne[1] != 1 || t.ne[2] != 1 || t.ne[3] != 1 || t.nb[0] != 4 || !scratch_add(n)) return nullptr;
        claimed[i] = 2;
        return t.host;
    }
    // Reshape3D(View1D(cache, T * d, off), hd, H, T): both at the view's address; the owner is a leaf over a registered buffer
    bool cache_view3d(int r3, uint64_t rows, int* owner, uint64_t* off) const {
        if (!is(r3, gc::RESHAPE)) return false;
        const int v = s0(r3);
        if (!is(v, gc::VIEW) || !packed(v, rows * mi.d, 1, 1) || !packed(r3, mi.hd, mi.H, rows) || !alias(r3, v)) return false;
        *owner = T[v].storage;
        *off = T[v].view_off;
        return (uint32_t)*owner < n_leafs && T[*owner].buf != 0;
    }

    bool match_layer(int x_out, uint32_t il, int* x_in) {
        const uint64_t d = mi.d, F = mi.F, hd = mi.hd, H = mi.H, n = mi.N;
        int32_t* W = &mi.weights[(size_t)il * W_PER_LAYER];
        // x_out = Add(MulMat(w2, Mul(Silu(MulMat(w1,h2)), MulMat(w3,h2))), inpFF)      llama.go:354-366
        if (!fresh(x_out, gc::ADD, d, n, 1)) return false;
        const int mm2 = s0(x_out), inpFF = s1(x_out);
        if (!fresh(mm2, gc::MUL_MAT, d, n, 1) || !weight(s0(mm2), F, d, true, &W[W_W2])) return false;
        const int gm = s1(mm2);
        if (!fresh(gm, gc::MUL, F, n, 1)) return false;
        const int sl = s0(gm), mm3 = s1(gm);
        if (!fresh(sl, gc::SILU, F, n, 1) || !fresh(mm3, gc::MUL_MAT, F, n, 1)) return false;
        const int mm1 = s0(sl);
        if (!fresh(mm1, gc::MUL_MAT, F, n, 1)) return false;
        if (!weight(s0(mm1), d, F, true, &W[W_W1]) || !weight(s0(mm3), d, F, true, &W[W_W3])) return false;
        const int h2 = s1(mm1);
        if (s1(mm3) != h2) return false;
        int xff;
        if (!norm_mul(h2, &xff, &W[W_FFN_NORM]) || xff != inpFF) return false;
        // inpFF = Add(MulMat(wo, A), inpSA)                                             llama.go:336-340
        if (!fresh(inpFF, gc::ADD, d, n, 1)) return false;
        const int mmo = s0(inpFF), inpSA = s1(inpFF);
        if (!fresh(mmo, gc::MUL_MAT, d, n, 1) || !weight(s0(mmo), d, d, true, &W[W_WO])) return false;
        // A = Cpy(Permute(KQV), new2D)                                                  llama.go:328-333
        const int A = s1(mmo);
        if (!is(A, gc::CPY) || !is(s0(A), gc::PERMUTE)) return false;
        const int Ap = s0(A), kqv = s0(Ap);
        // KQV = MulMat(VTrans, S);  VTrans = Cpy(Permute(Reshape3D(View1D(V))), new3D) llama.go:315-325
        if (!is(kqv, gc::MUL_MAT)) return false;
        const int vt = s0(kqv), S = s1(kqv);
        if (!is(vt, gc::CPY) || !is(s0(vt), gc::PERMUTE)) return false;
        const int Vp = s0(vt);
        // S = SoftMax(DiagMaskInf(Scale(KQ, sc), past))                                 llama.go:303-313
        if (!is(S, gc::SOFT_MAX) || !is(s0(S), gc::DIAG_MASK_INF)) return false;
        const int dm = s0(S);
        if (!is(s0(dm), gc::SCALE)) return false;
        const int scn = s0(dm), kq = s0(scn);
        if (!is(kq, gc::MUL_MAT)) return false;
        // KQ = MulMat(Permute(Rope(Reshape3D(View1D(K)), mode 1)), Permute(Rope(Cpy(MulMat(wq,h1), new3D), mode 0)))   llama.go:281-300
        const int Kp = s0(kq), Qp = s1(kq);
        if (!is(Kp, gc::PERMUTE) || !is(Qp, gc::PERMUTE) || !is(s0(Kp), gc::ROPE) || !is(s0(Qp), gc::ROPE)) return false;
        const int kr = s0(Kp), qr = s0(Qp), qc = s0(qr);
        // parameters: host-readable, and castable before they are cast
        const float* pastp = host_param(s1(dm), 1);
        const float* scp = host_param(s1(scn), 1);
        const float* kpar = host_param(s1(kr), 3);
        const float* qpar = host_param(s1(qr), 3);
        if (!pastp || !scp || !kpar || !qpar) return false;
        if (*scp != (float)(1.0 / sqrt((double)d / (double)H))) return false;
        for (int k = 0; k < 3; ++k)
            if (!gc::castable_u32(kpar[k]) || !gc::castable_u32(qpar[k])) return false;
        if (!gc::castable_u32(*pastp)) return false;
        const uint32_t p = (uint32_t)qpar[0];
        if ((uint32_t)kpar[0] != p || (uint32_t)*pastp != p) return false;
        if ((uint32_t)qpar[1] != hd || (uint32_t)kpar[1] != hd || (uint32_t)qpar[2] != 0 || (uint32_t)kpar[2] != 1) return false;
        const uint64_t Tn = (uint64_t)p + n;   // rows of the cache the attention reads
        if (Tn > mi.ctx || Tn > gc::MAX_ROPE_POSITIONS) return false;
        if (il + 1 == mi.L) mi.past = p;
        else if (mi.past != p) return false;
        // shapes, strides and addresses: the reference's constructors, nothing else.  Q/K Permute(0,2,1,3) of [hd,H,*] (llama.go:288, 297),
        // V Permute(1,2,0,3) (llama.go:319), KQV [hd,N,H] merged back with Permute(0,2,1,3) (llama.go:328); all K-contiguous copies
        const uint64_t e4 = 4, dB = d * 4, hB = hd * 4;
        if (!cpy_into_leaf(A, d, n, 1)) return false;
        if (!fresh(kqv, gc::MUL_MAT, hd, n, H) || !alias(Ap, kqv) || !shaped(Ap, hd, H, n, e4, hB * n, hB, dB * n)) return false;
        if (!cpy_into_leaf(vt, Tn, hd, H)) return false;
        int vo, ko;
        uint64_t voff, koff;
        if (!cache_view3d(s0(Vp), Tn, &vo, &voff) || !alias(Vp, s0(Vp)) || !shaped(Vp, Tn, hd, H, dB, e4, hB, dB * Tn)) return false;
        if (!fresh(kq, gc::MUL_MAT, Tn, n, H)) return false;
        for (const int i : {scn, dm, S})
            if (!alias(i, kq) || !packed(i, Tn, n, H)) return false;
        if (!cache_view3d(s0(kr), Tn, &ko, &koff) || !alias(kr, s0(kr)) || !packed(kr, hd, H, Tn)) return false;
        if (!alias(Kp, kr) || !shaped(Kp, hd, Tn, H, e4, dB, hB, dB * Tn)) return false;
        if (!cpy_into_leaf(qc, hd, H, n) || !alias(qr, qc) || !packed(qr, hd, H, n)) return false;
        if (!alias(Qp, qr) || !shaped(Qp, hd, n, H, e4, dB, hB, dB * n)) return false;
        const int mmq = s0(qc);
        if (!fresh(mmq, gc::MUL_MAT, d, n, 1) || !weight(s0(mmq), d, d, true, &W[W_WQ])) return false;
        const int h1 = s1(mmq);
        int xsa;
        if (!norm_mul(h1, &xsa, &W[W_ATTN_NORM]) || xsa != inpSA) return false;
        if (il + 1 == mi.L) { mi.kc_owner = ko; mi.vc_owner = vo; }
        else if (mi.kc_owner != ko || mi.vc_owner != vo) return false;
        if (ko == vo || koff != (uint64_t)il * mi.ctx * d || voff != koff) return false;
        // K / V stores: Cpy(MulMat(wk|wv, h1), View1D(cache, N * d, d * (il * ctx + past)))   llama.go:274-278.  They stand in front of the nodes
        // that read the rows: the K Rope (it rotates them in the cache) and the V^T copy.
        const uint64_t soff = d * ((uint64_t)il * mi.ctx + p);
        bool gotk = false, gotv = false;
        for (const Store& s : stores) {
            if (s.off != soff) continue;
            const int i = (int)s.cpy, dstv = s1(i), src = s0(i), own = T[dstv].storage;
            const bool k = own == ko;
            if ((!k && own != vo) || (k ? gotk : gotv)) return false;   // a second store into the same rows
            if (i > (k ? kr : vt) || src == mmq) return false;
            if (!packed(dstv, n * d, 1, 1) || !packed(i, n * d, 1, 1) || !alias(i, dstv)) return false;
            if (!fresh(src, gc::MUL_MAT, d, n, 1) || s1(src) != h1 || !weight(s0(src), d, d, true, &W[k ? W_WK : W_WV])) return false;
            claimed[i] = claimed[dstv] = 1;
            (k ? gotk : gotv) = true;
        }
        if (!gotk || !gotv) return false;
        *x_in = inpSA;
        return true;
    }

    bool run() {
        claimed.assign(total, 0);
        if (!run_pattern()) return false;
        for (uint32_t i = n_leafs; i < total; ++i)
            if (!claimed[i]) return false;  // a node outside the Eval pattern: run the graph node by node
        // LH_T_OUTPUT: the host wants to read this node back (in the reference every Tensor.Data is readable after GraphCompute, ml.go:1411-1528).
        // A fused plan materialises the final node and `embeddings` (llama.go:381, read at llama.go:414-419); any other flagged intermediate
        // never exists in it, so such a graph runs node by node.
        for (uint32_t i = n_leafs; i + 1 < total; ++i)
            if ((T[i].flags & LH_T_OUTPUT) && (int)i != mi.emb_node) return false;
        return true;
    }
    // the leaf of a cache: an owner over a registered f32 buffer whose own window lies inside it
    bool cache_leaf(int i, const BufInfo& b) const {
        const lh_tensor& t = T[i];
        return t.op == gc::NONE && at(i, i, 0) && b.dtype == 0 && t.nb[0] == 4 && t.ne[0] <= b.nfloats && t.ne[1] == 1 && t.ne[2] == 1 && t.ne[3] == 1;
    }
    bool run_pattern() {
        if (total == n_leafs) return false;
        const int fin = (int)total - 1;
        if (!is(fin, gc::MUL_MAT)) return false;
        const int wout = s0(fin);
        if (wout < 0 || (uint32_t)wout >= n_leafs) return false;
        mi.d = T[wout].ne[0];
        mi.V = T[wout].ne[1];
        mi.N = T[fin].ne[1];
        if (mi.N > gc::MAX_ROPE_POSITIONS) return false;   // (and no product of extents below can wrap 64 bits)
        if (!fresh(fin, gc::MUL_MAT, mi.V, mi.N, 1)) return false;
        // count layers by walking the residual chain down to GetRows
        std::vector<int> outs;
        {
            const int h = s1(fin);
            if (!is(h, gc::MUL) || !is(s1(h), gc::RMS_NORM)) return false;
            int cur = s0(s1(h));
            while (is(cur, gc::ADD)) {
                outs.push_back(cur);
                const int inpFF = s1(cur);
                if (!is(inpFF, gc::ADD)) return false;
                cur = s1(inpFF);
                if (outs.size() > 4096) return false;
            }
            if (!is(cur, gc::GET_ROWS) || outs.empty()) return false;
        }
        mi.L = (uint32_t)outs.size();
        mi.weights.assign((size_t)mi.L * W_PER_LAYER + W_TAIL, -1);
        int32_t* tail = &mi.weights[(size_t)mi.L * W_PER_LAYER];
        if (!weight(wout, mi.d, mi.V, true, &tail[W_OUTPUT])) return false;
        int x;
        if (!norm_mul(s1(fin), &x, &tail[W_NORM]) || x != outs[0]) return false;
        mi.emb_node = s1(fin);
        // head geometry from the last layer's KQV [hd, N, H], the FFN width from its w2; the context size from the extent of the V cache:
        // embd * layers * ctx floats (llama.go:93)
        {
            const int mmo = s0(s1(outs[0]));
            if (!is(mmo, gc::MUL_MAT)) return false;
            const int A = s1(mmo);
            if (!is(A, gc::CPY) || !is(s0(A), gc::PERMUTE)) return false;
            const int kqv = s0(s0(A));
            if (!is(kqv, gc::MUL_MAT)) return false;
            mi.hd = T[kqv].ne[0];
            mi.H = T[kqv].ne[2];
            if (mi.hd % 2 || (uint64_t)mi.hd * mi.H != mi.d) return false;   // Rope turns pairs (ml.go:2282)
            const int mm2 = s0(outs[0]);
            if (!is(mm2, gc::MUL_MAT) || s0(mm2) < 0) return false;
            mi.F = T[s0(mm2)].ne[0];
            const int vt = s0(kqv);
            if (!is(vt, gc::CPY) || !is(s0(vt), gc::PERMUTE) || !is(s0(s0(vt)), gc::RESHAPE) || !is(s0(s0(s0(vt))), gc::VIEW)) return false;
            const int own = T[s0(s0(s0(vt)))].storage;
            BufInfo b;
            if (!T[own].buf || !lookup(T[own].buf, &b)) return false;
            const uint64_t per = (uint64_t)mi.d * mi.L;
            if (b.nfloats % per || b.nfloats > MAX_CACHE_FLOATS || b.nfloats / per > 0xffffffffull) return false;
            mi.ctx = (uint32_t)(b.nfloats / per);
        }
        stores.clear();
        for (uint32_t i = n_leafs; i < total; ++i) {
            if (T[i].op != gc::CPY) continue;
            const int dst = T[i].src1;   // (arity 1: the structural check does not look at a Cpy's src1)
            if (dst >= (int)n_leafs && (uint32_t)dst < i && T[dst].op == gc::VIEW && T[T[dst].storage].buf) stores.push_back(Store{T[dst].view_off, i});
        }
        int xin = -1;
        for (uint32_t k = 0; k < mi.L; ++k) {
            const uint32_t il = mi.L - 1 - k;
            if (!match_layer(outs[k], il, &xin)) return false;
            if (il > 0 && xin != outs[k + 1]) return false;
        }
        // x_0 = GetRows(tok_embeddings, embd)                                         llama.go:239-244
        if (!fresh(xin, gc::GET_ROWS, mi.d, mi.N, 1)) return false;
        if (!weight(s0(xin), mi.d, mi.V, false, &tail[W_TOK_EMB])) return false;
        const float* ids = host_param(s1(xin), mi.N);
        if (!ids) return false;
        mi.tokens_leaf = s1(xin);
        mi.tokens.resize(mi.N);
        for (uint32_t i = 0; i < mi.N; ++i) {
            if (!gc::castable_u32(ids[i])) return false;
            mi.tokens[i] = (uint32_t)ids[i];  // ids travel as fp32 (ml.go:1739)
            if (mi.tokens[i] >= mi.V) return false;
        }
        BufInfo kb, vb;
        if (T[mi.kc_owner].buf == T[mi.vc_owner].buf || !lookup(T[mi.kc_owner].buf, &kb) || !lookup(T[mi.vc_owner].buf, &vb)) return false;
        if (vb.nfloats != kb.nfloats || !cache_leaf(mi.kc_owner, kb) || !cache_leaf(mi.vc_owner, vb)) return false;
        mi.wtype = wtype_seen < 0 ? 0 : wtype_seen;
        return true;
    }
};

struct ExtentLookup {
    const lh_buf_extent* bufs;
    uint32_t n;
    bool operator()(lh_buf id, BufInfo* out) const {
        for (uint32_t k = 0; k < n; ++k)
            if (bufs[k].id == id) { out->nfloats = bufs[k].nfloats; out->dtype = bufs[k].dtype; out->has_shape = false; return true; }
        return false;
    }
};

// lh_graph_match (include/llamahip.h): 1 accepted, 0 rejected, negative: graph_check_structure refuses the array
inline int graph_match(const lh_tensor* T, uint32_t n_leafs, uint32_t n_nodes, const lh_buf_extent* bufs, uint32_t n_bufs, lh_match_info* out) {
    if (n_bufs && !bufs) return LH_EINVAL;
    const int bad = gc::graph_check_structure(T, n_leafs, n_nodes, nullptr, 0);
    if (bad) return bad;
    Matcher<ExtentLookup> m(T, n_leafs, n_nodes, ExtentLookup{bufs, n_bufs});
    if (!m.run()) return 0;
    if (out) {
        const MatchInfo& mi = m.mi;
        out->N = mi.N; out->past = mi.past; out->V = mi.V; out->d = mi.d; out->H = mi.H; out->hd = mi.hd; out->L = mi.L; out->F = mi.F; out->ctx = mi.ctx;
        out->wtype = mi.wtype;
        out->kc_owner = mi.kc_owner; out->vc_owner = mi.vc_owner; out->tokens_leaf = mi.tokens_leaf; out->emb_node = mi.emb_node;
        out->n_weights = (uint32_t)mi.weights.size();
        for (uint32_t k = 0; out->weights && k < out->n_weights && k < out->cap_weights; ++k) out->weights[k] = mi.weights[k];
    }
    return 1;
}

}  // namespace gm
}  // namespace lh
