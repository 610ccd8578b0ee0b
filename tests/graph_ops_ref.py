"""Reference model of the node path of lh_graph_compute (csrc/graph.hip run_node, csrc/kernels_generic.h): which floats every implemented op
reads and writes, and what it writes, restated from the reference's compute functions in numpy / float64.  Independent of oracle/ and of
csrc/graph_check.h: the check is tested against this file (tests/test_graph_check_cpu.py), the kernels against run() and its bounds
(tests/test_gpu_node_ops.py).

Storage is modelled like Go slices: every owner is one flat array, every tensor a (owner, view_off, ne, nb) window into it.  Sizes of owners: a
registered buffer holds what Graph.bufs says, a host leaf its nelem floats (that many are uploaded), any other owner its own strided span.

Addressing, per op (ns = NB / 4; rows = ne1 * ne2 * ne3):
    GetRows       dst row i at i * NE0, table row r at r * NE0                                   ml.go:1748
    Mul           row i at i * NE0 on all three tensors                                          ml.go:1906
    Add           row j at j * ns1 on all three tensors, src1.nb0 must be 4                      ml.go:2523, 2564
    Silu          row j at j * ns1, both contiguous                                              ml.go:2605-2613, 2637
    Scale         dst row j at j * ns1, both contiguous, factor = src1[0]                        ml.go:2338-2346, 2353, 2371
    SoftMax       dst row j at j * ns1, both contiguous                                          ml.go:2438-2446, 2471
    DiagMaskInf   dst[k * ns2 + j * ns1 + i * ns0] for k < ne2 * ne3, i > past + j               ml.go:2391-2404
    RMSNorm       row (i1, i2, i3) through ns1..ns3 on both sides, elements adjacent             ml.go:1786, 1801
    Repeat        2-D: dst[(i * nr0 + k) * ns1 + j * nc0 * ns0 ...] = src0[k * ns1 ...]           ml.go:1849-1859
    Cpy           dst flat in (i3, i2, i1, i0) order, source through all four strides            ml.go:2141-2213 (three branches, one enumeration)
    Rope          pairs at i3 * ns3 + i2 * ns2 + i1 * ns1 + i0 * ns0 by SRC0's strides on both sides, i2 >= (mode ? past : 0)    ml.go:2274-2322
    MulMat        src0 row (i01, i02, i03), src1 row (ic, i02, i03), dst[i01 * ns0 + ic * ns1 + i02 * ns2 + i03 * ns3]   ml.go:1976-2098
Reshape / View / Permute / leafs run nothing (ml.go:1658-1663).

Shape rules (a graph that breaks one is `unsafe`: the reference halts or panics, or its kernel and ours would part ways):
    Mul, Add: three equal shapes (ml.go:1882, 2517).  Silu, Scale, SoftMax, RMSNorm, DiagMaskInf: dst.ne == src0.ne (ml.go:2603, 2335, 2436, 1755).
    GetRows: dst.ne0 == src0.ne0, dst.ne1 == nelem(src1), src0.nb0 == 4 (ml.go:1726).  Cpy: dst contiguous, equal nelem (ml.go:2116-2124).
    Repeat: ne2 == ne3 == 1 on both, dst sizes multiples of src0's, nb0 == 4 on both (ml.go:1825-1846).
    MulMat: equal ne0, ne2, ne3; nb0 == 4 on both; dst.ne == (src0.ne1, src1.ne1, src0.ne2, src0.ne3) (ml.go:290-318, 1950, 1967).
    Rope: src1 has 3 values, dims even, 0 < dims <= ne0, src0.nb0 == 4, dst is the ViewTensor of src0 it rotates - same base, same ne; its own
          strides are not read (ml.go:1016, 2259, 2282); past + ne2 < 2^32.
    Parameters the host casts to uint32 (DiagMaskInf past, Rope's three, GetRows ids) are host-readable, finite, in [0, 2^32); ids < src0.ne1.
    Every byte stride is a multiple of 4, no extent is 0 (we refuse empty tensors), leafs carry no op, every op has the sources it reads.
    Launch limits (32-bit counts of run_node and the kernels; possible only with zero strides or huge registered buffers): RMSNorm, SoftMax and
    GetRows take at most 2^31 - 1 rows (one workgroup each), MulMat 4 (2^31 - 1) outputs, DiagMaskInf ne2 * ne3 < 2^32 and past + ne1 <= 2^32.

Values and a-priori bounds, u = 2^-24 (one fp32 rounding is at most u relative):
    GetRows, Repeat, Cpy, DiagMaskInf   copies / constants: bit for bit.
    Mul, Add, Scale                     one IEEE fp32 operation: bit for bit against numpy's float32 arithmetic.
    Silu    silu_ref (kernels_common.h): den = fl32(1 + exp_f64(-x)) is one rounding, x / den a second: k = 2, |err| <= 2 u |y| (a slack of 2^-20
            relative covers the second-order terms and the f64 exp of another libm).  den overflows fp32 for x < -88.73: y = -0, as the reference.
    RMSNorm 3 u |y|: each square is rounded once in fp32 (ml.go:1792: the fp32 product rounds first) - relative error u of every term, hence of
            the sum, hence u / 2 of 1 / sqrt - the sum itself is f64; the scale's conversion to fp32 adds u, the product x * scale one more u.
            Squares that overflow fp32 make the mean inf, the scale 0 and every y of the row 0.
    SoftMax element i of a row of nc entries with maximum m: ((nc - 1) + |p_i - m| + 4) u y_i.  The fp32 sum of nc terms in any order carries at most
            (nc - 1) u; the fp32 subtraction p_i - m in front of the f64 exp carries u |p_i - m| into the exponent; one conversion of exp to fp32, one
            reciprocal, one product, and the conversions inside the sum: 4 u.  Per element: a tail probability is held as tightly as the peak.
            -inf entries give 0; a row of only -inf gives NaN (0 * (1 / 0)); a NaN or +inf anywhere in a row makes every entry NaN.
    Rope    rotation in f64 from f64 cos / sin, one rounding: u / 2 (|x0| + |x1|); cos / sin of another libm: bound 1.5 u (|x0| + |x1|).
    MulMat  16 u sum_k |a_k b_k|, the bound tests/test_gpu_matmul_routes.py holds g_mul_mat to.
"""
import ctypes as C
import struct

import numpy as np

U = 2.0 ** -24
NONE, ADD, MUL, REPEAT, SILU, RMS_NORM, MUL_MAT, SCALE, CPY, RESHAPE, VIEW, PERMUTE, GET_ROWS, DIAG_MASK_INF, SOFT_MAX, ROPE = \
    0, 2, 4, 10, 17, 19, 20, 21, 22, 23, 24, 25, 27, 28, 29, 30
ARITY = {NONE: 0, RESHAPE: 0, VIEW: 0, PERMUTE: 0, RMS_NORM: 1, REPEAT: 1, SILU: 1, CPY: 1, SOFT_MAX: 1,
         GET_ROWS: 2, MUL: 2, ADD: 2, SCALE: 2, DIAG_MASK_INF: 2, ROPE: 2, MUL_MAT: 2}
LH_OK, LH_EINVAL, LH_ENOMEM, LH_EHIP, LH_EUNSUPPORTED, LH_ENODEVICE, LH_ESHAPE = 0, -1, -2, -3, -4, -5, -6
F32_MAX = float(np.finfo(np.float32).max)
MAX_GRID = 2 ** 31 - 1   # workgroups of one launch


class LhTensor(C.Structure):  # struct lh_tensor (include/llamahip.h)
    _fields_ = [("op", C.c_uint8), ("dtype", C.c_uint8), ("flags", C.c_uint16), ("ne", C.c_uint32 * 4), ("nb", C.c_uint64 * 4),
                ("src0", C.c_int32), ("src1", C.c_int32), ("storage", C.c_int32), ("reserved", C.c_uint32), ("view_off", C.c_uint64),
                ("buf", C.c_uint64), ("host", C.POINTER(C.c_float))]


class LhBufExtent(C.Structure):  # struct lh_buf_extent
    _fields_ = [("id", C.c_uint64), ("nfloats", C.c_uint64), ("dtype", C.c_int)]


class T:
    __slots__ = ("op", "ne", "nb", "src0", "src1", "storage", "view_off", "buf", "host", "dtype", "flags")

    def __init__(self, op, ne, nb, src0=-1, src1=-1, storage=-1, view_off=0, buf=0, host=None):
        self.op, self.ne, self.nb, self.src0, self.src1 = op, list(ne), list(nb), src0, src1
        self.storage, self.view_off, self.buf, self.host, self.dtype, self.flags = storage, view_off, buf, host, 0, 0

    def copy(self):
        t = T(self.op, self.ne, self.nb, self.src0, self.src1, self.storage, self.view_off, self.buf, self.host)
        t.dtype, t.flags = self.dtype, self.flags
        return t


def ne4(ne):
    return list(ne) + [1] * (4 - len(ne))


def packed_nb(ne):
    nb = [4]
    for k in range(3):
        nb.append(nb[-1] * ne[k])
    return nb


class Graph:
    """Tensors in array order (leafs first).  Builders append; leafs must all be made before the first node (leaf() checks)."""

    def __init__(self):
        self.t, self.n_leafs, self.bufs = [], 0, {}
        self.counts = None   # (n_leafs, n_nodes) to hand over the C-ABI where they are NOT to describe the array (counts whose sum wraps)

    @property
    def total(self):
        return len(self.t)

    def copy(self):
        g = Graph()
        g.t, g.n_leafs, g.bufs, g.counts = [x.copy() for x in self.t], self.n_leafs, dict(self.bufs), self.counts
        return g

    def abi_counts(self):
        return self.counts or (self.n_leafs, self.total - self.n_leafs)

    # ---- leafs
    def _leaf(self, t):
        assert self.n_leafs == len(self.t), "leafs first"
        t.storage = len(self.t) if t.storage < 0 else t.storage
        self.t.append(t)
        self.n_leafs += 1
        return len(self.t) - 1

    def host(self, arr, ne=None):
        arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        ne = ne4(ne if ne is not None else [arr.size])
        assert int(np.prod(ne)) == arr.size
        return self._leaf(T(NONE, ne, packed_nb(ne), host=arr))

    def buffer(self, buf_id, nfloats, ne=None):
        """owner leaf over a registered buffer of nfloats floats"""
        self.bufs[buf_id] = (nfloats, 0)
        ne = ne4(ne if ne is not None else [nfloats])
        return self._leaf(T(NONE, ne, packed_nb(ne), buf=buf_id))

    def scratch(self, ne):
        ne = ne4(ne)
        return self._leaf(T(NONE, ne, packed_nb(ne)))

    # ---- nodes
    def node(self, op, ne, src0=-1, src1=-1, nb=None, like=None, off=0):
        """like = index of the tensor whose storage this node is a window of (view_off = that tensor's + off); None: the node owns new scratch"""
        ne = ne4(ne)
        t = T(op, ne, nb or packed_nb(ne), src0, src1)
        if like is None:
            t.storage = len(self.t)
        else:
            t.storage, t.view_off = self.t[like].storage, self.t[like].view_off + off
        self.t.append(t)
        return len(self.t) - 1

    def view(self, src, ne, nb=None, off=0, op=VIEW):
        return self.node(op, ne, src, -1, nb=nb, like=src, off=off)

    def permute(self, src, axes):
        """ml.go:786-845: ne[axes[k]] = src.ne[k]"""
        s = self.t[src]
        ne, nb = [0] * 4, [0] * 4
        for k in range(4):
            ne[axes[k]], nb[axes[k]] = s.ne[k], s.nb[k]
        return self.node(PERMUTE, ne, src, -1, nb=nb, like=src)

    def inplace(self, op, src, param=-1):
        s = self.t[src]
        return self.node(op, s.ne, src, param, nb=list(s.nb), like=src)

    def cpy(self, src, dst):
        d = self.t[dst]
        return self.node(CPY, d.ne, src, dst, nb=list(d.nb), like=dst)

    def into(self, op, dst, src0, src1=-1):
        """op whose result lands in the window `dst` (a view made before)"""
        d = self.t[dst]
        return self.node(op, d.ne, src0, src1, nb=list(d.nb), like=dst)

    # ---- C side
    def pack(self):
        """(lh_tensor array, lh_buf_extent array, n_bufs); host arrays stay referenced by the Graph"""
        arr = (LhTensor * max(1, len(self.t)))()
        for i, t in enumerate(self.t):
            fill_record(arr[i], t)
        ids = sorted(self.bufs)
        ext = (LhBufExtent * max(1, len(ids)))()
        for k, b in enumerate(ids):
            ext[k].id, ext[k].nfloats, ext[k].dtype = b, self.bufs[b][0], self.bufs[b][1]
        return arr, ext, len(ids)


def fill_record(r, t):
    r.op, r.dtype, r.flags = t.op & 0xff, t.dtype, t.flags
    for k in range(4):
        r.ne[k], r.nb[k] = t.ne[k] & 0xffffffff, t.nb[k] & 0xffffffffffffffff
    r.src0, r.src1, r.storage = t.src0, t.src1, t.storage
    r.view_off, r.buf = t.view_off & 0xffffffffffffffff, t.buf
    r.host = t.host.ctypes.data_as(C.POINTER(C.c_float)) if t.host is not None else None


# ---- sizes and reach ---------------------------------------------------------------------------------------------------------------------

def nelem(t):
    return t.ne[0] * t.ne[1] * t.ne[2] * t.ne[3]


def nrows(t):
    return t.ne[1] * t.ne[2] * t.ne[3]


def ns(t):
    return [b // 4 for b in t.nb]


def span(t):
    return 1 + sum((t.ne[k] - 1) * (t.nb[k] // 4) for k in range(4))


def contiguous(t):  # ml.go:206-211
    return t.nb[0] == 4 and t.nb[1] == t.nb[0] * t.ne[0] and t.nb[2] == t.nb[1] * t.ne[1] and t.nb[3] == t.nb[2] * t.ne[2]


def is_host_leaf(g, j):
    t = g.t[j]
    return t.op == NONE and t.storage == j and not t.buf and t.host is not None


def owner_size(g, i):
    """floats the owner i holds, or None when it names a buffer nobody registered"""
    t = g.t[i]
    if t.buf:
        return g.bufs[t.buf][0] if t.buf in g.bufs else None
    return nelem(t) if t.host is not None else span(t)


def castable(v):
    v = float(v)
    return v == v and 0.0 <= v < 4294967296.0


def op_reach(g, i):
    """[(tensor index, floats from that tensor's base the op's loops address, 'r' / 'w')] of node i by the addressing rules of the module
    docstring, in closed form (exact integers: ne up to 2^32, strides up to 2^61)."""
    t = g.t[i]
    a = g.t[t.src0] if t.src0 >= 0 else None
    b = g.t[t.src1] if t.src1 >= 0 else None
    op = t.op
    if op == GET_ROWS:
        ids = b.host
        top = int(max(ids[:nelem(b)])) if ids is not None and len(ids) else 0
        return [(t.src0, (top + 1) * a.ne[0], "r"), (t.src1, nelem(b), "r"), (i, nelem(b) * t.ne[0], "w")]
    if op == MUL:
        return [(t.src0, nelem(a), "r"), (t.src1, nelem(a), "r"), (i, nelem(a), "w")]
    if op == ADD:
        r = nrows(a)
        return [(j, (r - 1) * ns(x)[1] + a.ne[0], m) for j, x, m in ((t.src0, a, "r"), (t.src1, b, "r"), (i, t, "w"))]
    if op == SILU:
        r = nrows(a)
        return [(t.src0, (r - 1) * ns(a)[1] + a.ne[0], "r"), (i, (r - 1) * ns(t)[1] + a.ne[0], "w")]
    if op in (SCALE, SOFT_MAX):
        r = nrows(t)
        out = [(i, (r - 1) * ns(t)[1] + t.ne[0], "w")]
        return out + ([(t.src1, 1, "r")] if op == SCALE else [])
    if op == DIAG_MASK_INF:
        s = ns(t)
        return [(i, (t.ne[2] * t.ne[3] - 1) * s[2] + (t.ne[1] - 1) * s[1] + (t.ne[0] - 1) * s[0] + 1, "w"), (t.src1, 1, "r")]
    if op in (RMS_NORM, REPEAT):
        return [(t.src0, span(a), "r"), (i, span(t), "w")]
    if op == CPY:
        return [(t.src0, span(a), "r"), (i, nelem(a), "w")]
    if op == ROPE:
        return [(i, span(a), "w"), (t.src1, 3, "r")]             # src0's strides from the base the two share
    if op == MUL_MAT:
        return [(t.src0, span(a), "r"), (t.src1, span(b), "r"), (i, span(t), "w")]
    return []


def reach(g):
    """{node: {owner: (min offset, max offset)}} over what the node's op addresses, in floats from the owner's base"""
    out = {}
    for i in range(g.n_leafs, g.total):
        per = {}
        for j, n, _ in op_reach(g, i):
            o, lo = g.t[j].storage, g.t[j].view_off
            hi = lo + n - 1
            per[o] = (min(lo, per[o][0]), max(hi, per[o][1])) if o in per else (lo, hi)
        out[i] = per
    return out


def tensor_fault(g, i, n_leafs=None):
    """why tensor i alone makes the graph one we must refuse (structure, its own window, its op's rules and reach), or None"""
    n_leafs = g.n_leafs if n_leafs is None else n_leafs
    total = g.total
    t = g.t[i]
    if not (0 <= t.storage < total):
        return "storage out of range"
    if g.t[t.storage].storage != t.storage:
        return "owner is a view"
    if not (-1 <= t.src0 < total and -1 <= t.src1 < total):
        return "source out of range"
    if any(b % 4 for b in t.nb):
        return "stride not a multiple of 4"
    if any(n == 0 for n in t.ne):
        return "empty extent"
    if i < n_leafs:
        if t.op != NONE:
            return "leaf with an op"
    else:
        for s in (t.src0, t.src1):
            if s >= i and s >= n_leafs:
                return "node before its source"
        if t.op not in ARITY:
            return "unimplemented op"
        if (ARITY[t.op] >= 1 and t.src0 < 0) or (ARITY[t.op] >= 2 and t.src1 < 0):
            return "missing source"
    size = owner_size(g, t.storage)
    if size is None:
        return "unknown buffer"
    if t.view_off + span(t) > size:
        return "window leaves its owner"
    if i < n_leafs or ARITY[t.op] == 0:
        return None
    a = g.t[t.src0]
    b = g.t[t.src1] if ARITY[t.op] == 2 else None
    for x in (a, b):
        if x is not None and (any(n == 0 for n in x.ne) or any(s % 4 for s in x.nb) or not (0 <= x.storage < total)):
            return "operand is malformed"
    op = t.op
    same = lambda x, y: x.ne == y.ne
    if op == GET_ROWS:
        if t.ne[0] != a.ne[0] or t.ne[1] != nelem(b) or a.nb[0] != 4:
            return "GetRows dimensions"
        if not is_host_leaf(g, t.src1):
            return "GetRows ids not host-readable"
        if len(b.host) < nelem(b):
            return "GetRows ids shorter than nelem"
        if any(not castable(v) or int(v) >= a.ne[1] for v in b.host[:nelem(b)]):
            return "GetRows id outside the table"
    elif op in (MUL, ADD):
        if not (same(a, b) and same(a, t)):
            return "different shapes"
        if op == ADD and not (a.nb[0] == 4 and b.nb[0] == 4 and t.nb[0] == 4):
            return "Add rows not contiguous"
    elif op in (SILU, SCALE, SOFT_MAX):
        if not (contiguous(a) and contiguous(t) and same(a, t)):
            return "not contiguous / different shapes"
        if op == SCALE and nelem(b) != 1:
            return "Scale factor is no scalar"
    elif op == RMS_NORM:
        if not (same(a, t) and a.nb[0] == 4 and t.nb[0] == 4):
            return "RMSNorm shapes"
    elif op == REPEAT:
        if not (a.ne[2] == a.ne[3] == t.ne[2] == t.ne[3] == 1 and t.ne[0] % a.ne[0] == 0 and t.ne[1] % a.ne[1] == 0 and a.nb[0] == 4 and t.nb[0] == 4):
            return "Repeat shapes"
    elif op == CPY:
        if not (contiguous(t) and nelem(t) == nelem(a)):
            return "Cpy shapes"
    elif op == DIAG_MASK_INF:
        if not same(a, t) or nelem(b) != 1:
            return "DiagMaskInf shapes"
        if not is_host_leaf(g, t.src1) or not castable(b.host[0]):
            return "DiagMaskInf past cannot be cast"
    elif op == ROPE:
        if nelem(b) != 3 or not is_host_leaf(g, t.src1) or len(b.host) < 3:
            return "Rope parameters missing"
        if not all(castable(v) for v in b.host[:3]):
            return "Rope parameters cannot be cast"
        past, dims = int(b.host[0]), int(b.host[1])
        if dims == 0 or dims % 2 or dims > a.ne[0] or a.nb[0] != 4:
            return "Rope dims"
        if not (same(a, t) and a.storage == t.storage and a.view_off == t.view_off):
            return "Rope dst is not its source's view"
        if past + a.ne[2] >= 2 ** 32:
            return "Rope position wraps"
    elif op == MUL_MAT:
        if a.ne[0] != b.ne[0] or a.ne[2] != b.ne[2] or a.ne[3] != b.ne[3] or a.nb[0] != 4 or b.nb[0] != 4:
            return "MulMat operands"
        if t.ne != [a.ne[1], b.ne[1], a.ne[2], a.ne[3]]:
            return "MulMat dst shape"
    for j, n, _ in op_reach(g, i):
        x = g.t[j]
        size = owner_size(g, x.storage)
        if size is None or x.view_off + n > size:
            return f"op reaches past tensor {j}'s owner"
    # counts run_node and the kernels keep in 32 bits (a grid of at most 2^31 - 1 workgroups): beyond them rows would be skipped, not faulted
    if op in (RMS_NORM, SOFT_MAX) and nrows(t) > MAX_GRID or op == GET_ROWS and t.ne[1] > MAX_GRID:
        return "more rows than one launch has workgroups"
    if op == MUL_MAT and (nrows(a) * b.ne[1] + 3) // 4 > MAX_GRID:
        return "more outputs than one launch has waves"
    if op == DIAG_MASK_INF and (t.ne[2] * t.ne[3] >= 2 ** 32 or int(b.host[0]) + t.ne[1] > 2 ** 32):
        return "DiagMaskInf planes or past + rows wrap in 32 bits"
    return None


def graph_fault(g, n_leafs=None, n_nodes=None, only=None):
    """None when the model calls the graph safe, else the first reason.  only: the tensor indices to look at (the others are known good)."""
    nl = g.abi_counts()[0] if n_leafs is None else n_leafs
    nn = g.abi_counts()[1] if n_nodes is None else n_nodes
    if nl + nn >= 2 ** 31 or nl + nn != g.total:
        return "counts do not describe the array"
    for i in (range(g.total) if only is None else sorted(only)):
        why = tensor_fault(g, i, nl)
        if why:
            return f"tensor {i}: {why}"
    return None


def dependents(g, i):
    """tensors whose verdict can change when tensor i changes: i, what reads or writes through it, and - when i owns storage - every window
    into it and their users"""
    touched = {i} | {j for j, t in enumerate(g.t) if t.storage == i}
    users = {j for j, t in enumerate(g.t) if t.src0 in touched or t.src1 in touched}
    return touched | users


# ---- values --------------------------------------------------------------------------------------------------------------------------------

def _full_offsets(t):
    s = ns(t)
    i3, i2, i1, i0 = np.meshgrid(*(np.arange(t.ne[k], dtype=np.int64) for k in (3, 2, 1, 0)), indexing="ij", sparse=True)
    return t.view_off + i3 * s[3] + i2 * s[2] + i1 * s[1] + i0 * s[0]          # shape (ne3, ne2, ne1, ne0)


def _row_offsets(t, rows, nc, pitch):
    return t.view_off + np.arange(rows, dtype=np.int64)[:, None] * pitch + np.arange(nc, dtype=np.int64)[None, :]


class NodeResult:
    """offs: written offsets in the owner (flat int64); y32: the fp32 restatement's values there; y64 / bound: the float64 value and the a-priori
    bound of every written element (exact: bound 0, y32 is the contract bit for bit)"""

    def __init__(self, owner, offs, y32, y64=None, bound=None):
        self.owner, self.offs = owner, np.asarray(offs, dtype=np.int64).reshape(-1)
        self.y32 = np.asarray(y32, dtype=np.float32).reshape(-1)
        self.exact = y64 is None
        self.y64 = self.y32.astype(np.float64) if y64 is None else np.asarray(y64, dtype=np.float64).reshape(-1)
        self.bound = np.zeros(self.y64.shape) if bound is None else np.asarray(bound, dtype=np.float64).reshape(-1)


def silu64(x):
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        den = 1.0 + np.exp(-x64)
        den = np.where(den > F32_MAX * (1 + 2.0 ** -25), np.inf, den)          # fl32(den) overflows: the quotient is a signed zero
        return x64 / den


def softmax64(p):
    """rows of p (fp32) -> float64 probabilities by the rules of the module docstring, and the per-element bound"""
    p64 = p.astype(np.float64)
    nc = p.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = p64.max(axis=-1, keepdims=True)
        d = p64 - m
        e = np.where(np.isneginf(p64), 0.0, np.exp(d))
        y = e / e.sum(axis=-1, keepdims=True)
        bad = np.isnan(p64).any(axis=-1, keepdims=True) | np.isposinf(p64).any(axis=-1, keepdims=True) | np.isneginf(p64).all(axis=-1, keepdims=True)
        y = np.where(bad, np.nan, y)
        bound = ((nc - 1) + np.abs(np.where(np.isfinite(d), d, 0.0)) + 4) * U * np.where(bad, 0.0, y)
    return y, bound


def rms_norm64(x):
    """rows of x (fp32): squares rounded in fp32 first (ml.go:1792), summed in f64"""
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (x * x).astype(np.float32).astype(np.float64)
        mean = sq.sum(axis=-1, keepdims=True) / x.shape[-1]
        scale = 1.0 / np.sqrt(mean + 1e-5)
        y = x.astype(np.float64) * scale
    return y, 3 * U * np.abs(y)


def rope64(x0, x1, pos, i0, dims):
    theta = np.power(10000.0, -i0.astype(np.float64) / dims)
    c, s = np.cos(pos * theta), np.sin(pos * theta)
    a, b = x0.astype(np.float64), x1.astype(np.float64)
    bound = 1.5 * U * (np.abs(a) + np.abs(b))
    return a * c - b * s, a * s + b * c, bound


def exec_node(g, i, mem):
    """run node i on the owners' fp32 arrays `mem` (not modified); NodeResult or None for a node that runs nothing"""
    t = g.t[i]
    if t.op not in ARITY or ARITY[t.op] == 0:
        return None
    a = g.t[t.src0]
    b = g.t[t.src1] if ARITY[t.op] == 2 else None
    A = mem[a.storage]
    D = mem[t.storage]
    op = t.op
    with np.errstate(all="ignore"):
        if op == GET_ROWS:
            ids = mem[b.storage][b.view_off:b.view_off + nelem(b)].astype(np.uint32).astype(np.int64)
            nc = a.ne[0]
            src = a.view_off + ids[:, None] * nc + np.arange(nc)[None, :]
            return NodeResult(t.storage, _row_offsets(t, len(ids), nc, t.ne[0]), A[src])
        if op == MUL:
            n = nelem(a)
            x, y = A[a.view_off:a.view_off + n], mem[b.storage][b.view_off:b.view_off + n]
            return NodeResult(t.storage, t.view_off + np.arange(n), x * y)
        if op == ADD:
            r, nc = nrows(a), a.ne[0]
            x, y = A[_row_offsets(a, r, nc, ns(a)[1])], mem[b.storage][_row_offsets(b, r, nc, ns(b)[1])]
            return NodeResult(t.storage, _row_offsets(t, r, nc, ns(t)[1]), x + y)
        if op == SILU:
            r, nc = nrows(a), a.ne[0]
            x = A[_row_offsets(a, r, nc, ns(a)[1])]
            y = silu64(x)
            return NodeResult(t.storage, _row_offsets(t, r, nc, ns(t)[1]), y.astype(np.float32), y, 2 * U * (1 + 2.0 ** -20) * np.abs(y))
        if op == SCALE:
            offs = _row_offsets(t, nrows(t), t.ne[0], ns(t)[1])
            return NodeResult(t.storage, offs, D[offs] * mem[b.storage][b.view_off])
        if op == SOFT_MAX:
            offs = _row_offsets(t, nrows(t), t.ne[0], ns(t)[1])
            y, bound = softmax64(D[offs])
            return NodeResult(t.storage, offs, y.astype(np.float32), y, bound)
        if op == DIAG_MASK_INF:
            past = int(np.uint32(mem[b.storage][b.view_off]))
            s = ns(t)
            k, j, c = np.meshgrid(np.arange(t.ne[2] * t.ne[3]), np.arange(t.ne[1]), np.arange(t.ne[0]), indexing="ij")
            hit = c > past + j
            offs = (t.view_off + k * s[2] + j * s[1] + c * s[0])[hit]
            return NodeResult(t.storage, offs, np.full(offs.shape, -np.inf, np.float32))
        if op == RMS_NORM:
            src, dst = _full_offsets(a), _full_offsets(t)
            y, bound = rms_norm64(A[src])
            return NodeResult(t.storage, dst, y.astype(np.float32), y, bound)
        if op == REPEAT:
            sa, sd = ns(a), ns(t)
            row, col = np.meshgrid(np.arange(t.ne[1]), np.arange(t.ne[0]), indexing="ij")
            src = a.view_off + (row % a.ne[1]) * sa[1] + (col % a.ne[0])
            return NodeResult(t.storage, t.view_off + row * sd[1] + col * sd[0], A[src])
        if op == CPY:
            src = np.broadcast_to(_full_offsets(a), (a.ne[3], a.ne[2], a.ne[1], a.ne[0])).reshape(-1)
            return NodeResult(t.storage, t.view_off + np.arange(src.size), A[src])
        if op == ROPE:
            P = mem[b.storage][b.view_off:b.view_off + 3]
            past, dims, mode = int(np.uint32(P[0])), int(np.uint32(P[1])), int(np.uint32(P[2]))
            first = 0 if mode == 0 else past
            if first >= a.ne[2]:
                return NodeResult(t.storage, np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0), np.zeros(0))
            s = ns(a)                                            # src0's NE and NB on both sides (ml.go:2274-2281)
            i3, i2, i1, i0 = np.meshgrid(np.arange(a.ne[3]), np.arange(first, a.ne[2]), np.arange(a.ne[1]), np.arange(0, dims, 2), indexing="ij")
            off = t.view_off + i3 * s[3] + i2 * s[2] + i1 * s[1] + i0 * s[0]
            pos = (past + i2 if mode == 0 else i2).astype(np.float64)
            y0, y1, bound = rope64(D[off], D[off + 1], pos, i0, dims)
            offs = np.concatenate([off.reshape(-1), off.reshape(-1) + 1])
            y = np.concatenate([y0.reshape(-1), y1.reshape(-1)])
            return NodeResult(t.storage, offs, y.astype(np.float32), y, np.concatenate([bound.reshape(-1)] * 2))
        if op == MUL_MAT:
            B = mem[b.storage]
            sa, sb, sd = ns(a), ns(b), ns(t)
            K = a.ne[0]
            offs, ys, bounds = [], [], []
            for i3 in range(a.ne[3]):
                for i2 in range(a.ne[2]):
                    wa = A[a.view_off + i3 * sa[3] + i2 * sa[2] + np.arange(a.ne[1])[:, None] * sa[1] + np.arange(K)[None, :]].astype(np.float64)
                    xb = B[b.view_off + i3 * sb[3] + i2 * sb[2] + np.arange(b.ne[1])[:, None] * sb[1] + np.arange(K)[None, :]].astype(np.float64)
                    ys.append((xb @ wa.T).reshape(-1))                                       # [ic][i01]
                    bounds.append(16 * U * (np.abs(xb) @ np.abs(wa).T).reshape(-1))
                    offs.append((t.view_off + i3 * sd[3] + i2 * sd[2] + np.arange(b.ne[1])[:, None] * sd[1] + np.arange(a.ne[1])[None, :] * sd[0]).reshape(-1))
            y = np.concatenate(ys)
            return NodeResult(t.storage, np.concatenate(offs), y.astype(np.float32), y, np.concatenate(bounds))
    raise AssertionError(f"op {op}")


SENTINEL_BITS = 0x7FC5A5A5          # a quiet NaN with a payload no kernel produces: what unwritten scratch and buffer floats hold


def sentinel(n):
    return np.full(n, SENTINEL_BITS, dtype=np.uint32).view(np.float32)


class Run:
    pass


def run(g, inputs=None):
    """inputs: {buffer id: fp32 array of the buffer's floats}.  Returns Run with mem (owner -> fp32 array, the fp32 restatement's final state),
    written (owner -> bool mask) and nodes (node index -> NodeResult)."""
    inputs = inputs or {}
    r = Run()
    r.mem, r.written, r.nodes = {}, {}, {}
    for i, t in enumerate(g.t):
        if t.storage != i:
            continue
        n = owner_size(g, i)
        if t.buf:
            r.mem[i] = np.array(inputs[t.buf], dtype=np.float32).reshape(-1).copy()
            assert r.mem[i].size == n
        elif t.host is not None:
            r.mem[i] = t.host[:n].copy()
        else:
            r.mem[i] = sentinel(n)
        r.written[i] = np.zeros(n, dtype=bool)
    for i in range(g.n_leafs, g.total):
        res = exec_node(g, i, r.mem)
        if res is None:
            continue
        assert res.offs.size == 0 or (res.offs.min() >= 0 and res.offs.max() < r.mem[res.owner].size), f"node {i} writes outside its owner"
        r.mem[res.owner][res.offs] = res.y32
        r.written[res.owner][res.offs] = True
        r.nodes[i] = res
    return r


def bound(res):
    """the a-priori bound of every written element of a NodeResult (zeros: bit for bit)"""
    return res.bound


def violations(got32, res):
    """indices (into res.offs) where the fp32 values `got32` at res.offs break the node's contract"""
    got = np.asarray(got32, dtype=np.float32).reshape(-1)
    if res.exact:
        return np.nonzero(got.view(np.uint32) != res.y32.view(np.uint32))[0] if not np.isnan(res.y32).any() else \
            np.nonzero(~((got.view(np.uint32) == res.y32.view(np.uint32)) | (np.isnan(got) & np.isnan(res.y32))))[0]
    g64 = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(g64 - res.y64) <= res.bound) | (np.isnan(g64) & np.isnan(res.y64)) | (np.isinf(res.y64) & (g64 == res.y64))
    return np.nonzero(~ok)[0]


def judge(g, inputs, model, got):
    """What a device run must satisfy, as a list of complaints (empty: fine).  got: {owner index: the owner's whole registered buffer read back as
    fp32}.  Every element a node wrote is inside that node's contract; every other float of every buffer keeps the bits it had in `inputs`."""
    out = []
    for node, res in model.nodes.items():
        if res.owner not in got:
            out.append(f"node {node}: its destination is no registered buffer")
            continue
        bad = violations(got[res.owner][res.offs], res)
        if bad.size:
            k = bad[0]
            out.append(f"node {node} (op {g.t[node].op}): {bad.size} of {res.offs.size} elements outside the bound, first at offset {res.offs[k]}: "
                       f"got {got[res.owner][res.offs[k]]!r}, float64 {res.y64[k]!r}, bound {res.bound[k]:.3e}")
    for owner, arr in got.items():
        before = np.asarray(inputs[g.t[owner].buf], dtype=np.float32).view(np.uint32)
        stray = np.nonzero((arr.view(np.uint32) != before) & ~model.written[owner])[0]
        if stray.size:
            out.append(f"{stray.size} floats outside what the ops write changed, first at offset {stray[0]} of tensor {owner}'s buffer")
    return out


# ---- the stand-alone checker's file format (tests/graph_check_main.cpp) -------------------------------------------------------------------
F_NONE, F_OP, F_SRC0, F_SRC1, F_STORAGE, F_NE, F_NB, F_VIEW_OFF, F_HOST_NULL, F_HOST_VALUE, F_COUNTS, F_FLAGS, F_SWAP = 0, 1, 2, 3, 4, 5, 9, 13, 14, 15, 16, 17, 18


def graph_bytes(g):
    """n_leafs, n_nodes, n_bufs, n_vals (u32 each); records of 96 bytes whose host field holds 1 + the index of the first value (0: no host data);
    buffer extents (u64 id, u64 nfloats, i32 dtype, i32 0); values (f32)"""
    vals, recs = [], b""
    for t in g.t:
        r = LhTensor()
        host, t_host = 0, t.host
        if t_host is not None:
            host = 1 + sum(len(v) for v in vals)
            vals.append(t_host)
        t.host = None
        fill_record(r, t)
        t.host = t_host
        raw = bytearray(bytes(r))
        raw[88:96] = struct.pack("<Q", host)
        recs += bytes(raw)
    ids = sorted(g.bufs)
    flat = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, np.float32)
    out = struct.pack("<IIII", g.n_leafs, g.total - g.n_leafs, len(ids), flat.size) + recs
    for b in ids:
        out += struct.pack("<QQii", b, g.bufs[b][0], g.bufs[b][1], 0)
    return out + flat.tobytes()
