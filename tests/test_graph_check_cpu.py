"""not-gpu: lh_graph_check (csrc/graph_check.h) - what lh_graph_compute refuses before it enqueues anything - against the reference model of op
addressing (tests/graph_ops_ref.py), without a device.

  accept corpus   the Eval graph of the host mirror (real lh_tensor records with storage, view_off and buffers), every graph tests/test_gpu_ops.py
                  builds, the view cases of tests/test_gpu_node_ops.py: all accepted, and the model's own run stays inside every owner.
  mutant corpus   deterministic and exhaustive: one field of one tensor at a time.  SOUNDNESS: every mutant the model calls unsafe is refused.
                  CAP: at most 2 % of the mutants the model calls safe are refused, and at least a fifth of all mutants are safe.
  bounds          the a-priori bounds of RMSNorm and SoftMax hold for fp32 restatements in four summation orders and fail four wrong kernels.
  sanitizers      tests/graph_check_main.cpp (graph_check.h and graph_match.h behind its own main) built with -fsanitize=address,undefined runs the
                  same corpora as a child process: no report, verdicts of lh_graph_check and of lh_graph_match identical to the library's.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import graph_ops_ref as R
import node_op_cases as cases
from llama_go_amd.mlapi import SHAPES, HParams, make_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U


# ---- the libraries -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    hip.lh_graph_check.restype = C.c_int
    hip.lh_graph_check.argtypes = [C.POINTER(R.LhTensor), C.c_uint32, C.c_uint32, C.POINTER(R.LhBufExtent), C.c_uint32, C.c_char_p, C.c_uint64]
    hip.lh_graph_match.restype = C.c_int
    hip.lh_graph_match.argtypes = [C.POINTER(R.LhTensor), C.c_uint32, C.c_uint32, C.POINTER(R.LhBufExtent), C.c_uint32, C.c_void_p]
    return hip


@pytest.fixture(scope="module")
def mirror(lib):
    import llama_go_amd as pkg
    m = C.CDLL(pkg.LIBLLAMAGO)
    m.llamago_EvalGraphRecords.restype = C.c_int
    m.llamago_EvalGraphRecords.argtypes = [C.POINTER(HParams), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(R.LhTensor), C.c_uint32, C.POINTER(C.c_uint32),
                                           C.POINTER(R.LhBufExtent), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    m.llamago_GraphRecords.restype = C.c_int
    m.llamago_GraphRecords.argtypes = [C.c_void_p, C.POINTER(R.LhTensor), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    return m


BIG_LEAF = 2 ** 20


class HostStandIn:
    """what the model needs of a large leaf's host data: that it is there, and its length; the record points at one float, which nobody reads"""

    def __init__(self, n):
        self.n, self.one = n, np.zeros(1, np.float32)
        self.ctypes = self.one.ctypes

    def __len__(self):
        return self.n


def match_verdict(lib, g, packed=None, counts=None):
    arr, ext, nb = packed or g.pack()
    nl, nn = counts or g.abi_counts()
    return lib.lh_graph_match(arr, nl, nn, ext, nb, None)


def check(lib, g, n_leafs=None, n_nodes=None, packed=None):
    arr, ext, nb = packed or g.pack()
    msg = C.create_string_buffer(256)
    rc = lib.lh_graph_check(arr, g.abi_counts()[0] if n_leafs is None else n_leafs, g.abi_counts()[1] if n_nodes is None else n_nodes, ext, nb, msg, 256)
    return rc, msg.value.decode()


def graph_of_records(arr, n, n_leafs, ext=None, n_ext=0):
    g = R.Graph()
    g.n_leafs = n_leafs
    for i in range(n):
        r = arr[i]
        t = R.T(r.op, list(r.ne), list(r.nb), r.src0, r.src1, r.storage, r.view_off, r.buf)
        t.dtype, t.flags = r.dtype, r.flags
        if r.host:
            # the values of a large data leaf are never read by the check or by the model's reach: a stand-in of the same length, not a copy
            cnt = R.nelem(t)
            t.host = np.ctypeslib.as_array(r.host, shape=(cnt,)).copy() if cnt <= BIG_LEAF else HostStandIn(cnt)
        g.t.append(t)
    for k in range(n_ext):
        g.bufs[ext[k].id] = (ext[k].nfloats, ext[k].dtype)
    return g


def eval_graph(mirror, shape, N, past, ctx=64):
    hp = make_hparams(**SHAPES[shape], ctx=ctx)
    nl, nb, nv = C.c_uint32(), C.c_uint32(), C.c_uint32()
    n = mirror.llamago_EvalGraphRecords(C.byref(hp), ctx, N, past, None, 0, C.byref(nl), None, 0, C.byref(nb), None, 0, C.byref(nv))
    assert n > 0
    arr, ext, vals = (R.LhTensor * n)(), (R.LhBufExtent * nb.value)(), (C.c_float * max(1, nv.value))()
    assert mirror.llamago_EvalGraphRecords(C.byref(hp), ctx, N, past, arr, n, C.byref(nl), ext, nb.value, C.byref(nb), vals, nv.value, C.byref(nv)) == n
    return graph_of_records(arr, n, nl.value, ext, nb.value)


def params(test):
    """{argnames: argvalues} of a test function's parametrize marks"""
    return {m.args[0]: m.args[1] for m in test.pytestmark if m.name == "parametrize"}


def ops_graphs(mirror):
    """every graph tests/test_gpu_ops.py builds: its own parametrize lists (read from the module, so that they cannot drift) through the same
    constructors, flattened by the host mirror without a device.  The check looks at shapes, strides and parameter leafs only, so data leafs stay
    as NewTensor allocates them."""
    import test_gpu_ops as ops
    from llama_go_amd.mlapi import load_product
    ml = load_product()

    def leaf(*shape):                                            # numpy shape [.., ne1, ne0], as leaf() of test_gpu_ops.py
        return ml.NewTensor(None, tuple(reversed(shape)))

    def values(v):
        v = np.asarray(v, dtype=np.float32)
        return ml.NewTensor(None, tuple(reversed(v.shape)), data=v)

    def attention(T, N, H, hd, past):
        d = H * hd
        K3 = ml.Permute(None, ml.Reshape3D(None, leaf(T * d), hd, H, T), 0, 2, 1, 3)
        Q3 = ml.Permute(None, ml.Copy(None, leaf(N, d), ml.NewTensor(None, (hd, H, N))), 0, 2, 1, 3)
        S = ml.SoftMax(None, ml.DiagMaskInf(None, ml.Scale(None, ml.MulMat(None, K3, Q3), ml.NewFP32(None, 1.0 / np.sqrt(hd))), past))
        VT = ml.Copy(None, ml.Permute(None, ml.Reshape3D(None, leaf(T * d), hd, H, T), 1, 2, 0, 3), ml.NewTensor(None, (T, hd, H)))
        return [S, ml.Copy(None, ml.Permute(None, ml.MulMat(None, VT, S), 0, 2, 1, 3), ml.NewTensor(None, (d, N)))]

    def full_7b(K, M, N):                                        # four products over shared leafs in one graph
        W, X = leaf(M, K), leaf(N, K)
        return [ml.MulMat(None, W, X), ml.MulMat(None, leaf(M, K), leaf(N, K)), ml.MulMat(None, leaf(M, K), X), ml.MulMat(None, W, leaf(N, K))]

    def rms(d, N):
        cur = ml.RMSNorm(None, leaf(N, d))
        return [ml.Mul(None, ml.Repeat(None, leaf(d), cur), cur)]

    def rope(mode, past, N):
        return [ml.Rope(None, leaf(N if mode == 0 else past + N, 3, 128), past, 128, mode)]

    def permuted_copy(perm):
        p = ml.Permute(None, leaf(4, 6, 8), *perm)
        return [ml.Copy(None, p, ml.NewTensor(None, ml.shape(p)[0][:3]))]

    def cache():
        c = leaf(80)
        return [ml.Copy(None, leaf(2, 16), ml.View1D(None, c, 32, 32)), ml.Copy(None, ml.View1D(None, c, 80, 0), ml.NewTensor(None, (80,)))]

    builders = {}
    for K, M, N in params(ops.test_mul_mat_weights)["K,M,N"]:
        builders[f"mul_mat_weights_{K}_{M}_{N}"] = lambda K=K, M=M, N=N: [ml.MulMat(None, leaf(M, K), leaf(N, K))]
    full = params(ops.test_mul_mat_full_7b_matrices_exact_properties)
    for K, M in full["K,M"]:
        for N in full["N"]:
            builders[f"mul_mat_full_7b_{K}_{M}_{N}"] = lambda K=K, M=M, N=N: full_7b(K, M, N)
    for a in params(ops.test_attention_chain)["T,N,H,hd,past"]:
        builders["attention_chain_" + "_".join(map(str, a))] = lambda a=a: attention(*a)
    builders["attention_chain"] = lambda: attention(7, 2, 3, 32, 5)          # the mutant corpus's
    for d, N in params(ops.test_rms_norm_repeat_mul)["d,N"]:
        builders[f"rms_norm_repeat_mul_{d}_{N}"] = lambda d=d, N=N: rms(d, N)
    for a in params(ops.test_rope)["mode,past,N"]:
        builders["rope_" + "_".join(map(str, a))] = lambda a=a: rope(*a)
    builders["silu_add_scale"] = lambda: [ml.Add(None, ml.Mul(None, ml.Silu(None, leaf(3, 1000)), leaf(3, 1000)), leaf(3, 1000))]
    builders["get_rows"] = lambda: [ml.GetRows(None, leaf(50, 64), values([3, 49, 0, 3]))]
    for perm in [(1, 2, 0, 3), (0, 2, 1, 3), (2, 0, 1, 3)]:
        builders["copy_perm" + "".join(map(str, perm))] = lambda perm=perm: permuted_copy(perm)
    builders["view_copy_into_cache"] = cache
    import test_gpu_node_ops as node_ops                         # its Rope graphs for the checker are built through this API too
    rope_marks = params(node_ops.test_rope_on_strided_views_bit_for_bit_against_the_checker)
    for layout in rope_marks["layout"]:
        for mode, n2, past in rope_marks["mode,n2,past"]:
            axes = node_ops.ROPE_LAYOUTS[layout]
            builders[f"rope_checker_{layout}_{mode}_{n2}_{past}"] = lambda s=(2, n2, 128), axes=axes, past=past, mode=mode: \
                [node_ops.rope_checker_graph(ml, None, np.zeros(s, np.float32), axes, past, mode)]
    out = {}
    for name, build in builders.items():
        gr = ml.NewGraph()
        for t in build():
            ml.BuildForwardExpand(gr, t)
        nl, nv = C.c_uint32(), C.c_uint32()
        n = mirror.llamago_GraphRecords(gr, None, 0, C.byref(nl), None, 0, C.byref(nv))
        assert n > 0
        arr, vals = (R.LhTensor * n)(), (C.c_float * max(1, nv.value))()
        assert mirror.llamago_GraphRecords(gr, arr, n, C.byref(nl), vals, nv.value, C.byref(nv)) == n
        out[name] = graph_of_records(arr, n, nl.value)
        ml.FreeGraph(gr)
    return out


def seven_ops_graph():
    """seven nodes, one each of the ops the attention chain does not use: GetRows, RMSNorm, Repeat, Mul, Silu, Add, Rope (behind a Reshape)"""
    g = R.Graph()
    r = np.random.default_rng(9)
    table, ids = g.host(r.standard_normal((11, 8)), (8, 11)), g.host([3, 0, 10], (3,))
    gamma, bias, par = g.host(r.standard_normal(8), (8,)), g.host(r.standard_normal((3, 8)), (8, 3)), g.host([2, 4, 0])
    x = g.node(R.GET_ROWS, (8, 3), table, ids)
    n = g.node(R.RMS_NORM, (8, 3), x)
    rep = g.node(R.REPEAT, (8, 3), gamma, n)
    m = g.node(R.MUL, (8, 3), rep, n)
    s = g.node(R.SILU, (8, 3), m)
    a = g.node(R.ADD, (8, 3), s, bias)
    v = g.view(a, (4, 2, 3), op=R.RESHAPE)
    g.inplace(R.ROPE, v, par)
    return g


@pytest.fixture(scope="module")
def corpus(mirror):
    acc = {}
    for shape in ("tiny", "small"):
        for N, past in ((1, 0), (1, 23), (8, 0), (40, 17)):
            acc[f"eval_{shape}_N{N}_past{past}"] = eval_graph(mirror, shape, N, past)
    acc.update({"ops_" + k: v for k, v in ops_graphs(mirror).items()})
    acc.update({"view_" + c.name: c.g for c in cases.accepted_cases()})
    acc["view_cpy_4100x4100"] = cases.big_cpy_case().g
    acc["raw_abi"] = cases.raw_abi_graph()[0]
    acc["seven_ops"] = seven_ops_graph()
    return acc


# ---- accept corpus -------------------------------------------------------------------------------------------------------------------------

def test_accept_corpus_is_accepted_and_in_range_by_the_model(lib, corpus):
    assert len(corpus) >= 120
    for name, g in corpus.items():
        rc, msg = check(lib, g)
        assert rc == 0, f"{name}: refused with {rc}: {msg}"
        assert R.graph_fault(g) is None, f"{name}: the model calls it unsafe: {R.graph_fault(g)}"
        sizes = {i: R.owner_size(g, i) for i, t in enumerate(g.t) if t.storage == i}
        for node, per in R.reach(g).items():
            for owner, (lo, hi) in per.items():
                assert 0 <= lo <= hi < sizes[owner], (name, node, owner, lo, hi, sizes[owner])


def test_model_run_touches_what_its_closed_form_reach_says(corpus):
    """graph_ops_ref.run enumerates every offset an op reads or writes; op_reach states the furthest one in closed form - the two are written
    separately and must agree on every view case (writes: never beyond, and equal for every op that writes its whole window)."""
    seen = set()
    for c in cases.accepted_cases():
        res = R.run(c.g, c.inputs)
        for i, nr in res.nodes.items():
            t = c.g.t[i]
            closed = [n for j, n, m in R.op_reach(c.g, i) if j == i and m == "w"][0]
            if nr.offs.size == 0:
                continue
            hi = int(nr.offs.max()) - t.view_off + 1
            assert hi <= closed, (c.name, i)
            if t.op not in (R.DIAG_MASK_INF, R.ROPE):
                assert hi == closed, (c.name, i, hi, closed)
            seen.add(t.op)
    assert seen == {R.ADD, R.MUL, R.REPEAT, R.SILU, R.RMS_NORM, R.MUL_MAT, R.SCALE, R.CPY, R.GET_ROWS, R.DIAG_MASK_INF, R.SOFT_MAX, R.ROPE}


def test_refused_representatives_are_refused_and_unsafe_by_the_model(lib):
    reps = cases.refused_cases()
    assert len(reps) >= 12
    for name, g, bad, words in reps:
        rc, msg = check(lib, g)
        assert rc < 0, f"{name} was accepted"
        assert words in msg, (name, msg)
        assert R.graph_fault(g) is not None, f"{name}: the model calls it safe"


# ---- mutant corpus -------------------------------------------------------------------------------------------------------------------------

INT32_MIN = -2 ** 31


def u32(v):
    return v & 0xffffffff


def mutations(g):
    """[(tensor, field, value)] - one field of one tensor at a time (fields: graph_ops_ref.F_*)"""
    total = g.total
    view = next((i for i, t in enumerate(g.t) if t.storage != i), 0)
    out = [(0, R.F_NONE, 0)]
    for i, t in enumerate(g.t):
        for f in (R.F_SRC0, R.F_SRC1):
            out += [(i, f, u32(v)) for v in (-2, -1, INT32_MIN, i, total - 1, total)]
        out += [(i, R.F_STORAGE, u32(v)) for v in (-1, total, view)]
        for k in range(4):
            out += [(i, R.F_NE + k, u32(v)) for v in (0, t.ne[k] - 1, t.ne[k] + 1, 2 ** 32 - 1)]
            out += [(i, R.F_NB + k, v & (2 ** 64 - 1)) for v in (0, t.nb[k] - 4, t.nb[k] + 4, t.nb[k] + 1, 2 ** 63)]
        size = R.owner_size(g, t.storage)
        out += [(i, R.F_VIEW_OFF, size - R.span(t) + 1), (i, R.F_VIEW_OFF, 2 ** 64 - 1)]
        out += [(i, R.F_OP, v) for v in range(256)]
        # mutations that keep the graph valid: the stride of a dimension of one element, a window moved inside its owner, flags, equal-shape sources swapped
        for k in range(4):
            if t.ne[k] == 1:
                out += [(i, R.F_NB + k, v) for v in sorted({4 << s for s in range(0, 40)} | {t.nb[k] * m for m in (2, 3, 5, 7)} | {t.nb[k] + 4 * a for a in (2, 3, 5, 100, 1000, 10 ** 6)})]
        slack = size - R.span(t)
        out += [(i, R.F_VIEW_OFF, v) for v in sorted({0, slack, slack // 2, slack // 3, min(slack, 1), min(slack, 2), min(slack, 5), max(slack - 1, 0)})]
        out += [(i, R.F_FLAGS, v) for v in range(16)]
        if t.src0 >= 0 and t.src1 >= 0:
            out.append((i, R.F_SWAP, 0))
        if t.host is not None and any(u.src1 == i and u.op in (R.SCALE, R.DIAG_MASK_INF, R.ROPE, R.GET_ROWS) for u in g.t):
            out.append((i, R.F_HOST_NULL, 0))
            is_ids = any(u.src1 == i and u.op == R.GET_ROWS for u in g.t)
            rows = next((g.t[u.src0].ne[1] for u in g.t if u.src1 == i and u.op == R.GET_ROWS), 0)
            values = (-1.0, float(rows), float("nan")) if is_ids else (-1.0, float("nan"), float("inf"), 2.0 ** 32, 2.0 ** 31)
            for k in range(min(len(t.host), 3)):
                out += [(i, R.F_HOST_VALUE, (k << 32) | struct.unpack("<I", struct.pack("<f", v))[0]) for v in values]
    out += [(0, R.F_COUNTS, (a << 32) | b) for a, b in ((2 ** 32 - 1, 1), (2 ** 31, 2 ** 31), (2 ** 32 - 1, 2 ** 32 - 1), (1, 2 ** 32 - 1), (2 ** 31, 0), (0, 2 ** 31))]
    return out


def s32(v):
    return v - 2 ** 32 if v >= 2 ** 31 else v


class Mutated:
    """apply one mutation to the model's tensor and to the packed record, undo on exit"""

    def __init__(self, g, arr, mut):
        self.g, self.arr, self.mut = g, arr, mut

    def __enter__(self):
        i, f, v = self.mut
        g, t, r = self.g, self.g.t[i], self.arr[i]
        self.saved = t.copy()
        self.saved_host = None
        self.counts = (g.n_leafs, g.total - g.n_leafs)
        if f == R.F_OP:
            t.op = v
        elif f == R.F_SRC0:
            t.src0 = s32(v)
        elif f == R.F_SRC1:
            t.src1 = s32(v)
        elif f == R.F_STORAGE:
            t.storage = s32(v)
        elif R.F_NE <= f < R.F_NE + 4:
            t.ne[f - R.F_NE] = v
        elif R.F_NB <= f < R.F_NB + 4:
            t.nb[f - R.F_NB] = v
        elif f == R.F_VIEW_OFF:
            t.view_off = v
        elif f == R.F_HOST_NULL:
            t.host = None
        elif f == R.F_HOST_VALUE:
            self.saved_host = t.host.copy()
            t.host.view(np.uint32)[v >> 32] = v & 0xffffffff
        elif f == R.F_COUNTS:
            self.counts = (v >> 32, v & 0xffffffff)
        elif f == R.F_FLAGS:
            t.flags = v
        elif f == R.F_SWAP:
            t.src0, t.src1 = t.src1, t.src0
        R.fill_record(r, t)
        return self

    def __exit__(self, *exc):
        i = self.mut[0]
        if self.saved_host is not None:
            self.g.t[i].host[:] = self.saved_host
        self.g.t[i] = self.saved
        R.fill_record(self.arr[i], self.saved)


def mutant_graphs(mirror):
    return {"eval_tiny_N3": eval_graph(mirror, "tiny", 3, 0), "attention_chain": ops_graphs(mirror)["attention_chain"], "seven_ops": seven_ops_graph()}


def classify(lib, g, muts, full=False):
    """[(library's return code, the model's reason or None)] per mutation.  The model looks at the tensors the mutation can reach only; full: and
    proves on the way that looking at every tensor gives the same verdict"""
    arr, ext, nb = g.pack()
    assert R.graph_fault(g) is None
    out = []
    msg = C.create_string_buffer(256)
    for mut in muts:
        with Mutated(g, arr, mut) as m:
            rc = lib.lh_graph_check(arr, m.counts[0], m.counts[1], ext, nb, msg, 256)
            if mut[1] == R.F_COUNTS:
                why = "counts wrap" if sum(m.counts) >= 2 ** 31 else None
            else:
                why = R.graph_fault(g, only=R.dependents(g, mut[0]) | self_before(m))
                if full:
                    assert (why is None) == (R.graph_fault(g) is None), (mut, why, R.graph_fault(g))
        out.append((rc, why))
    return out


def self_before(m):
    """what depended on the tensor BEFORE the mutation (a source or storage index that moved away leaves its old users to be looked at too)"""
    i = m.mut[0]
    now = m.g.t[i]
    m.g.t[i] = m.saved
    dep = R.dependents(m.g, i)
    m.g.t[i] = now
    return dep


@pytest.fixture(scope="module")
def verdicts(lib, mirror):
    out = {}
    for name, g in mutant_graphs(mirror).items():
        muts = mutations(g)
        out[name] = (g, muts, classify(lib, g, muts, full=g.total < 40))
    return out


def test_mutants_soundness_and_cap(verdicts):
    report = []
    for name, (g, muts, res) in verdicts.items():
        unsafe_accepted = [(m, why) for m, (rc, why) in zip(muts, res) if why is not None and rc == 0]
        assert not unsafe_accepted, f"{name}: {len(unsafe_accepted)} unsafe mutants accepted, first {unsafe_accepted[0]}"
        safe = [(m, rc) for m, (rc, why) in zip(muts, res) if why is None]
        refused_safe = [(m, rc) for m, rc in safe if rc != 0]
        report.append(f"{name}: {len(muts)} mutants, {len(safe)} safe, {len(muts) - len(safe)} unsafe, {len(refused_safe)} safe ones refused")
        assert all(rc < 0 for rc, why in res if why is not None)
        assert len(safe) * 5 >= len(muts), report[-1]
        assert len(refused_safe) * 50 <= len(safe), report[-1] + f", e.g. {refused_safe[:5]}"
    print("\n".join(report))


def test_model_alone_classifies_the_corpus_meaningfully(verdicts):
    """the cap means something only if the model calls a fair share of every KIND of mutation safe and unsafe: sizes, strides, offsets and ops
    have both safe and unsafe mutants; indices outside the array and counts that wrap are always unsafe"""
    for name, (g, muts, res) in verdicts.items():
        kinds = {}
        for (i, f, v), (rc, why) in zip(muts, res):
            k = "ne" if R.F_NE <= f < R.F_NE + 4 else "nb" if R.F_NB <= f < R.F_NB + 4 else f
            kinds.setdefault(k, [0, 0])[why is not None] += 1
        for k in ("ne", "nb", R.F_VIEW_OFF, R.F_OP, R.F_SRC0, R.F_HOST_VALUE):
            assert kinds[k][0] > 0 and kinds[k][1] > 0, (name, k, kinds[k])
        assert kinds[R.F_COUNTS][0] == 0 and kinds[R.F_STORAGE][1] > 0
    g, muts, res = verdicts["seven_ops"]
    by = {m: why for m, (rc, why) in zip(muts, res)}
    total = g.total
    assert by[(total - 1, R.F_SRC1, u32(-1))] and by[(total - 1, R.F_SRC0, u32(-2))] and by[(total - 1, R.F_NE, 0)]
    assert by[(total - 1, R.F_OP, R.VIEW)] is None and by[(0, R.F_FLAGS, 3)] is None


# ---- the same corpora under sanitizers, stand-alone -------------------------------------------------------------------------------------

def test_corpora_under_address_and_undefined_sanitizers(lib, mirror, corpus, verdicts, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "graph_check_main")
    # the runtimes are linked statically: the child then starts whatever its environment preloads, and the environment is passed on as it is
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "llama.go_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "graph_check_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]
    graphs, muts, want = [], [], []
    for name, g in corpus.items():
        if name.startswith("eval_small") or any(R.nelem(t) > BIG_LEAF for t in g.t[:g.n_leafs]):
            continue                                             # (the large ones add bytes, not paths)
        rc, _ = check(lib, g)
        graphs.append(g); muts.append((len(graphs) - 1, 0, R.F_NONE, 0)); want.append((rc, match_verdict(lib, g)))
    for _, g, _, _ in cases.refused_cases():
        rc, _ = check(lib, g)
        graphs.append(g); want.append((rc, match_verdict(lib, g)))
        muts.append((len(graphs) - 1, 0, R.F_COUNTS, (g.counts[0] << 32) | g.counts[1]) if g.counts else (len(graphs) - 1, 0, R.F_NONE, 0))
    for name, (g, ms, res) in verdicts.items():
        graphs.append(g)
        muts += [(len(graphs) - 1, i, f, v) for i, f, v in ms]
        arr, ext, nb = g.pack()
        for mut, (rc, _) in zip(ms, res):
            with Mutated(g, arr, mut) as m:
                want.append((rc, match_verdict(lib, g, (arr, ext, nb), m.counts)))
    assert sum(m == 1 for _, m in want) > 1000 and sum(m == 0 for _, m in want) > 1000    # the matcher's verdicts: both sorts, many
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(graphs)))
        for g in graphs:
            fh.write(R.graph_bytes(g))
        fh.write(struct.pack("<I", len(muts)))
        for gi, i, f, v in muts:
            fh.write(struct.pack("<IIIIQ", gi, i, f, 0, v))
    run = subprocess.run([exe, path], capture_output=True, text=True)
    if run.returncode != 0 and "runtime error" not in run.stderr and ("link order" in run.stderr or "Shadow memory" in run.stderr or "ReserveShadowMemoryRange" in run.stderr):
        pytest.skip("the sanitizer runtime refuses to start here: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, f"exit {run.returncode}:\n{run.stderr[-3000:]}"
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    got = [tuple(int(x) for x in ln.split()) for ln in run.stdout.splitlines()]
    assert len(got) == len(want)
    bad = [k for k in range(len(got)) if got[k] != want[k]]
    assert not bad, f"{len(bad)} verdicts differ, first: mutation {muts[bad[0]]} stand-alone {got[bad[0]]} library {want[bad[0]]} (lh_graph_check, lh_graph_match)"


# ---- bound self-checks -------------------------------------------------------------------------------------------------------------------

def sum_orders(v, dt=np.float32):
    """sums of the last axis in precision dt: left to right, reversed, pairwise, and the kernels' order (lane t takes t, t + 256, ..; 64 lanes fold as a tree;
    four waves are added)"""
    v = v.astype(dt)
    n = v.shape[-1]

    def seq(a):
        s = np.zeros(a.shape[:-1], dt)
        for k in range(a.shape[-1]):
            s = (s + a[..., k]).astype(dt)
        return s

    def pairwise(a):
        while a.shape[-1] > 1:
            if a.shape[-1] % 2:
                a = np.concatenate([a, np.zeros(a.shape[:-1] + (1,), dt)], axis=-1)
            a = (a[..., 0::2] + a[..., 1::2]).astype(dt)
        return a[..., 0]

    def tree(a):
        pad = (-n) % 256
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), dt)], axis=-1).reshape(a.shape[:-1] + (-1, 4, 64))
        lanes = seq(np.moveaxis(a, -3, -1))                      # per thread: its strided elements in order
        waves = pairwise(lanes)                                  # 64 lanes, butterfly
        return ((waves[..., 0] + waves[..., 1]).astype(dt) + (waves[..., 2] + waves[..., 3]).astype(dt)).astype(dt)

    return {"left_to_right": seq(v), "reversed": seq(v[..., ::-1]), "pairwise": pairwise(v), "tree_4x64": tree(v)}


def softmax32(p, total):
    with np.errstate(all="ignore"):
        m = p.max(axis=-1, keepdims=True)
        e = np.where(np.isneginf(p), np.float32(0), np.exp((p - m).astype(np.float32).astype(np.float64)).astype(np.float32)).astype(np.float32)
        inv = (np.float32(1) / total(e)).astype(np.float32)
        return (e * inv[..., None]).astype(np.float32), e


def finite_rows(x):
    return x[np.isfinite(x).all(axis=-1) | (np.isneginf(x).any(axis=-1) & ~np.isneginf(x).all(axis=-1) & ~np.isnan(x).any(axis=-1) & ~np.isposinf(x).any(axis=-1))]


def inside(y32, y64, bound):
    with np.errstate(invalid="ignore"):
        return bool(np.all((np.abs(y32.astype(np.float64) - y64) <= bound) | (np.isnan(y32) & np.isnan(y64))))


@pytest.mark.parametrize("nc", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_softmax_bound_holds_for_every_summation_order_and_fails_wrong_kernels(nc):
    p = finite_rows(cases.softmax_rows(nc, cases.rng(1, nc)))
    y64, bound = R.softmax64(p)
    for name in ("left_to_right", "reversed", "pairwise", "tree_4x64"):
        y32, _ = softmax32(p, lambda e, name=name: sum_orders(e)[name])
        assert inside(y32, y64, bound), (nc, name)
    if nc < 63:
        return
    seq = lambda e: sum_orders(e)["left_to_right"]
    # one element dropped from the sum.  Which one matters: the LAST term of row 0 is ~1e-26 of the sum, and no bound on the outputs can see a
    # loop that stops one short there; so the mutant loses the largest term of each row, the drop a per-element bound must catch
    def dropped(e):
        e = e.copy()
        e[np.arange(e.shape[0]), e.argmax(axis=-1)] = 0
        return seq(e)
    assert not inside(softmax32(p, dropped)[0], y64, bound)
    if nc > 256:
        # the maximum taken over the first 256 entries only: softmax is shift-invariant, so this shows only where the peak beyond them is more than
        # 88.7 above it and exp overflows fp32 (the true row is ~ one-hot).  That takes this crafted input: the rows of softmax_rows spread over
        # +-30, and the GPU cases use those rows only - their tails would underflow fp32 at such a spread, which the relative bound has no term for -
        # so on the device such a kernel is caught by reading g_soft_max (one loop bound, nc, for both passes), not by tests/test_gpu_node_ops.py
        q = p.copy()
        q[:, nc - 1] = np.where(np.isfinite(q[:, nc - 1]), np.float32(130.0), q[:, nc - 1])
        y64q, boundq = R.softmax64(q)
        with np.errstate(all="ignore"):
            m = q[:, :256].max(axis=-1, keepdims=True)
            e = np.where(np.isneginf(q), 0, np.exp((q - m).astype(np.float32).astype(np.float64))).astype(np.float32)   # exp(+big) overflows fp32
            bad = (e * (np.float32(1) / seq(e))[:, None]).astype(np.float32)
        assert not inside(bad, y64q, boundq)


@pytest.mark.parametrize("n", [1, 100, 256, 257, 4096])
def test_rms_norm_bound_holds_for_every_summation_order_and_fails_wrong_kernels(n):
    x = cases.rms_rows(n)
    y64, bound = R.rms_norm64(x)
    with np.errstate(all="ignore"):
        sq = (x * x).astype(np.float32)

        def kernel(total):
            mean = total.astype(np.float64) / n
            scale = (1.0 / np.sqrt(mean + 1e-5)).astype(np.float32)
            return (x * scale[:, None]).astype(np.float32)

        s64 = sq.astype(np.float64)
        for name, total in sum_orders(s64, np.float64).items():      # the kernel's sum is f64, in the 4 x 64-lane tree order
            assert inside(kernel(total), y64, bound), (n, name)
        if n >= 100:
            assert not inside(kernel(s64[:, :-1].sum(axis=-1)), y64, bound)                  # one element dropped from the sum
            assert not inside(kernel((x.astype(np.float64) ** 2).sum(axis=-1)) * np.float32(1 + 8 * U), y64, bound)   # a scale 8 u off


def buffers_after(case, model, rewrite):
    """the registered buffers as a device would hand them back: the model's fp32 state, then rewrite(owner arrays) plays the wrong kernel"""
    got = {i: model.mem[i].copy() for i, t in enumerate(case.g.t) if t.storage == i and t.buf}
    rewrite(got)
    return got


def test_mask_off_by_one_and_wrong_row_pitch_are_caught_by_the_device_comparison():
    """graph_ops_ref.judge - what tests/test_gpu_node_ops.py applies to the buffers read back - passes the model's own fp32 state and fails a
    DiagMaskInf that masks `i >= past + j` instead of `>` and an Add that puts its rows at NE0 pitch where ns1 is due"""
    c = next(c for c in cases.accepted_cases() if c.name == "diag_mask_9x4x3_past5")
    model = R.run(c.g, c.inputs)
    assert R.judge(c.g, c.inputs, model, buffers_after(c, model, lambda got: None)) == []
    node = max(model.nodes)
    t = c.g.t[node]
    s = R.ns(t)
    k, j, i = np.meshgrid(np.arange(t.ne[2]), np.arange(t.ne[1]), np.arange(t.ne[0]), indexing="ij")

    def off_by_one(got):
        got[t.storage][(t.view_off + k * s[2] + j * s[1] + i * s[0])[i >= 5 + j]] = -np.inf
    assert any("outside what the ops write" in p for p in R.judge(c.g, c.inputs, model, buffers_after(c, model, off_by_one)))

    c = next(c for c in cases.accepted_cases() if c.name == "add_kv_slot_rows")
    model = R.run(c.g, c.inputs)
    assert R.judge(c.g, c.inputs, model, buffers_after(c, model, lambda got: None)) == []
    node = max(model.nodes)
    t, res = c.g.t[node], model.nodes[max(model.nodes)]

    def flat_rows(got):
        got[t.storage][:] = np.asarray(c.inputs[c.g.t[t.storage].buf], np.float32)                   # the destination as it was
        got[t.storage][t.view_off + np.arange(48)] = res.y32                           # rows at a pitch of ne0 = 16, not 40
    problems = R.judge(c.g, c.inputs, model, buffers_after(c, model, flat_rows))
    assert any("outside the bound" in p for p in problems) and any("outside what the ops write" in p for p in problems), problems
