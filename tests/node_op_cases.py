"""The graphs tests/test_gpu_node_ops.py sends through the node path and tests/test_graph_check_cpu.py requires lh_graph_check to accept: every
generic kernel on views inside larger registered buffers (filled with graph_ops_ref.sentinel where no input lies), at the smallest shapes that
cross the kernels' edges (256 threads, 64 lanes, grid-stride loops).  refused_cases(): one graph per hole the node path used to have; every one of
them must be refused on the host.  Pure numpy: no library, no GPU."""
import numpy as np

import graph_ops_ref as R
from graph_ops_ref import Graph

PAD = 7   # floats of sentinel in front of every window, so that a write below a window's base shows


class Case:
    def __init__(self, name, g, inputs):
        self.name, self.g, self.inputs = name, g, inputs

    def __repr__(self):
        return self.name


def nb_of(ne, nb=None):
    return list(nb) if nb else R.packed_nb(R.ne4(ne))


class B:
    """builder: registered buffers first (src / dst / host), then windows into them and the nodes"""

    def __init__(self):
        self.g, self.inputs, self.next = Graph(), {}, 1

    def buf(self, nfloats):
        i = self.g.buffer(self.next, nfloats)
        self.inputs[self.next] = R.sentinel(nfloats)
        self.next += 1
        return i

    def src(self, ne, values, nb=None, tail=5):
        """a new buffer holding `values` (C order = (i3, i2, i1, i0)) in the window (ne, nb) at PAD, sentinel around"""
        t = R.T(0, R.ne4(ne), nb_of(ne, nb), view_off=PAD)
        leaf = self.buf(PAD + R.span(t) + tail)
        offs = np.broadcast_to(R._full_offsets(t), tuple(reversed(R.ne4(ne)))).reshape(-1)
        self.inputs[self.g.t[leaf].buf][offs] = np.asarray(values, dtype=np.float32).reshape(-1)
        return leaf

    def dst(self, ne, nb=None, tail=5):
        return self.buf(PAD + R.span(R.T(0, R.ne4(ne), nb_of(ne, nb))) + tail)

    def window(self, leaf, ne, nb=None, off=PAD, op=R.VIEW):
        return self.g.view(leaf, ne, nb=nb, off=off, op=op)

    def case(self, name):
        return Case(name, self.g, self.inputs)


def rng(*seed):
    return np.random.default_rng(list(seed))


def softmax_rows(nc, r):
    rows = r.uniform(-30, 30, (7, nc)).astype(np.float32)
    rows[0, 0] = 30.0
    rows[0, nc - 1] = -30.0 if nc > 1 else 30.0          # tail e^-60 ~ 1e-26
    rows[3, nc // 2:] = -np.inf                          # -inf tail (nc = 1: the whole row)
    rows[4, :] = -np.inf
    rows[5, nc - 1] = np.nan
    rows[6, nc // 3] = np.inf
    return rows


def rms_rows(n):
    x = (rng(3, n).standard_normal((5, n)) * 3).astype(np.float32)
    x[2] *= np.float32(1e-20)          # eps dominates
    x[3] *= np.float32(1e18)           # squares up to ~1e38: the top of fp32's range
    x[4] *= np.float32(1e20)           # squares beyond it: the fp32 product rounds to inf first (ml.go:1792), the mean is inf, the scale 0
    return x


SILU_SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 90.0, -90.0, -88.0, -87.5, 88.0, 1e-30, -1e-30]


def accepted_cases():
    cases = []
    # ---- SoftMax, in place on a contiguous window: 3 ordinary rows, then -inf tail, all -inf, NaN in the last place, +inf
    for nc in (1, 63, 64, 65, 255, 256, 257, 1000):
        b = B()
        leaf = b.src((nc, 7), softmax_rows(nc, rng(1, nc)))
        b.g.inplace(R.SOFT_MAX, b.window(leaf, (nc, 7)))
        cases.append(b.case(f"softmax_nc{nc}"))
    # ---- DiagMaskInf, in place; one window with a row pitch wider than the row
    for nc, nr, nz, past in ((1, 1, 1, 0), (9, 4, 3, 5), (300, 2, 2, 298), (8, 8, 1, 0)):
        b = B()
        pitch = nc + 3 if nc == 9 else nc
        nb = [4, pitch * 4, pitch * nr * 4, pitch * nr * nz * 4]
        leaf = b.src((nc, nr, nz), rng(2, nc).standard_normal((nz, nr, nc)), nb=nb)
        p = b.g.host([past])
        b.g.inplace(R.DIAG_MASK_INF, b.window(leaf, (nc, nr, nz), nb=nb), p)
        cases.append(b.case(f"diag_mask_{nc}x{nr}x{nz}_past{past}"))
    # ---- RMSNorm: rows of 1 .. 4096 floats with extreme rows; permuted 3-D and 4-D sources
    for n in (1, 100, 256, 257, 4096):
        b = B()
        s, d = b.src((n, 5), rms_rows(n)), b.dst((n, 5))
        b.g.into(R.RMS_NORM, b.window(d, (n, 5)), b.window(s, (n, 5)))
        cases.append(b.case(f"rms_norm_n{n}"))
    for name, ne, perm in (("rms_norm_permuted3d", (100, 3, 5, 1), (0, 2, 1, 3)), ("rms_norm_4d", (65, 3, 2, 2), (0, 1, 2, 3))):
        b = B()
        s = b.src(ne, rng(4, ne[0]).standard_normal(tuple(reversed(ne))))
        pne = [0] * 4
        for k in range(4):
            pne[perm[k]] = ne[k]
        d = b.dst(pne)
        sw = b.g.permute(b.window(s, ne), perm)
        b.g.into(R.RMS_NORM, b.window(d, pne), sw)
        cases.append(b.case(name))
    # ---- Repeat (2-D broadcast); the destination of one case has a row pitch wider than its rows
    for (nc0, nr0), (nc, nr) in (((5, 1), (5, 4)), ((1, 3), (7, 3)), ((3, 2), (9, 6)), ((4096, 1), (4096, 3))):
        b = B()
        dnb = [4, (nc + 2) * 4, (nc + 2) * nr * 4, (nc + 2) * nr * 4] if nc == 9 else None
        s, d = b.src((nc0, nr0), rng(5, nc).standard_normal((nr0, nc0))), b.dst((nc, nr), dnb)
        b.g.into(R.REPEAT, b.window(d, (nc, nr), nb=dnb), b.window(s, (nc0, nr0)))
        cases.append(b.case(f"repeat_{nc0}x{nr0}_to_{nc}x{nr}"))
    # ---- Add: KV-slot rows (3 rows of 16 in a pitch of 40) on src0 and dst, src1 packed; a contiguous 3-D case
    b = B()
    slot = [4, 160, 480, 480]
    r = rng(6)
    s0, s1, d = b.src((16, 3), r.standard_normal((3, 16)), nb=slot), b.src((16, 3), r.standard_normal((3, 16))), b.dst((16, 3), slot)
    b.g.into(R.ADD, b.window(d, (16, 3), nb=slot), b.window(s0, (16, 3), nb=slot), b.window(s1, (16, 3)))
    cases.append(b.case("add_kv_slot_rows"))
    b = B()
    ne = (257, 3, 2)
    s0, s1, d = b.src(ne, r.standard_normal((2, 3, 257))), b.src(ne, r.standard_normal((2, 3, 257))), b.dst(ne)
    b.g.into(R.ADD, b.window(d, ne), b.window(s0, ne), b.window(s1, ne))
    cases.append(b.case("add_3d"))
    # ---- Mul, Silu, Scale: 3-D contiguous, 1000 and 257 columns
    for nc in (1000, 257):
        ne = (nc, 3, 2)
        r = rng(7, nc)
        b = B()
        s0, s1, d = b.src(ne, r.standard_normal((2, 3, nc)) * 4), b.src(ne, r.standard_normal((2, 3, nc))), b.dst(ne)
        b.g.into(R.MUL, b.window(d, ne), b.window(s0, ne), b.window(s1, ne))
        cases.append(b.case(f"mul_3d_nc{nc}"))
        b = B()
        x = r.uniform(-90, 90, (2, 3, nc)).astype(np.float32)
        x[np.abs(x + 88.7) < 0.2] = -80.0                   # keep clear of the one input where fl32(1 + e^-x) turns inf
        x[0, 0, :len(SILU_SPECIALS)] = SILU_SPECIALS
        s, d = b.src(ne, x), b.dst(ne)
        b.g.into(R.SILU, b.window(d, ne), b.window(s, ne))
        cases.append(b.case(f"silu_3d_nc{nc}"))
        for f in ((0.125,) if nc == 1000 else (0.0, -1.0, np.inf)):
            b = B()
            x = r.standard_normal((2, 3, nc)).astype(np.float32)
            x[0, 0, :4] = [0.0, -0.0, np.inf, np.nan]
            s = b.src(ne, x)
            p = b.g.host([f])
            b.g.inplace(R.SCALE, b.window(s, ne), p)
            cases.append(b.case(f"scale_3d_nc{nc}_by_{f}"))
    # ---- Cpy: bulk (contiguous source), rows (nb0 == 4), element gather (nb0 != 4), from 4-D sources into a View1D slot at an offset
    ne = (4, 6, 8, 2)
    for perm in ((0, 1, 2, 3), (1, 2, 0, 3), (0, 2, 1, 3), (2, 0, 1, 3), (0, 1, 3, 2)):
        b = B()
        s = b.src(ne, rng(8).standard_normal(tuple(reversed(ne))))
        d = b.buf(600)
        sw = b.g.permute(b.window(s, ne), perm)
        b.g.cpy(sw, b.window(d, (384,), off=100))
        cases.append(b.case("cpy_perm" + "".join(map(str, perm))))
    # ---- GetRows: widths 1, 255, 257; repeated ids, the first and the last row of the table
    for nc in (1, 255, 257):
        b = B()
        s = b.src((nc, 11), rng(9, nc).standard_normal((11, nc)))
        ids = b.g.host([3, 10, 0, 3, 3, 10])
        d = b.dst((nc, 6))
        b.g.into(R.GET_ROWS, b.window(d, (nc, 6)), b.window(s, (nc, 11)), ids)
        cases.append(b.case(f"get_rows_nc{nc}"))
    # ---- Rope: both modes, dims = 64 of 128 (upper half untouched), 4-D, rows with a gap between them; mode 1 with past >= ne2 writes nothing
    for mode, n2, past in ((0, 3, 0), (0, 3, 5), (0, 3, 2047), (1, 7, 5), (1, 7, 0), (1, 7, 7), (1, 3, 2047)):
        b = B()
        ne = (128, 2, n2, 2)
        nb = [4, 130 * 4, 130 * 2 * 4, 130 * 2 * n2 * 4]
        s = b.src(ne, rng(10, mode, past).standard_normal((2, n2, 2, 128)), nb=nb)
        p = b.g.host([past, 64, mode])
        b.g.inplace(R.ROPE, b.window(s, ne, nb=nb), p)
        cases.append(b.case(f"rope_mode{mode}_n{n2}_past{past}"))
    # Rope on a permuted view whose result is a ViewTensor with packed strides of its own (ml.go:1016): the source's strides address both sides
    b = B()
    ne = (128, 3, 2)
    s = b.src(ne, rng(10, 99).standard_normal((2, 3, 128)))
    p = b.g.host([5, 64, 0])
    pw = b.g.permute(b.window(s, ne), (0, 2, 1, 3))          # ne = (128, 2, 3): three positions, ns1 > ns2
    b.g.node(R.ROPE, b.g.t[pw].ne, pw, p, like=pw)
    cases.append(b.case("permuted_rope_packed_result"))
    # ---- g_mul_mat on strided batches: K3 . Q3 of the attention (llama.go:281-300), and a weight whose rows have a pitch wider than K
    T_, N_ = 7, 2
    for H in (1, 3):
        for hd in (32, 100):
            b = B()
            r = rng(11, H, hd)
            k, q = b.src((hd, H, T_), r.standard_normal((T_, H, hd))), b.src((hd, H, N_), r.standard_normal((N_, H, hd)))
            d = b.dst((T_, N_, H))
            K3 = b.g.permute(b.window(k, (hd, H, T_), op=R.RESHAPE), (0, 2, 1, 3))
            Q3 = b.g.permute(b.window(q, (hd, H, N_), op=R.RESHAPE), (0, 2, 1, 3))
            b.g.into(R.MUL_MAT, b.window(d, (T_, N_, H)), K3, Q3)
            cases.append(b.case(f"mul_mat_kq_H{H}_hd{hd}"))
    b = B()
    r = rng(12)
    wnb = [4, 108 * 4, 108 * 5 * 4, 108 * 5 * 4]
    w, x, d = b.src((100, 5), r.standard_normal((5, 100)), nb=wnb), b.src((100, 3), r.standard_normal((3, 100))), b.dst((5, 3))
    b.g.into(R.MUL_MAT, b.window(d, (5, 3)), b.window(w, (100, 5), nb=wnb), b.window(x, (100, 3)))
    cases.append(b.case("mul_mat_row_pitch"))
    return cases


def big_cpy_case():
    """ne = (4100, 4100): 16.8M elements, more than 65535 x 256, so that the grid-stride loop of grid_for runs its second lap"""
    b = B()
    n = 4100
    x = (np.arange(n * n, dtype=np.int64) % 8191).astype(np.float32)
    s = b.src((n, n), x, tail=3)
    d = b.buf(n * n + 2 * PAD)
    b.g.cpy(b.window(s, (n, n)), b.window(d, (n * n,)))
    return b.case("cpy_4100x4100")


def raw_abi_graph():
    """the well-formed graph of tests/test_gpu_abi.py::test_graph_compute_through_the_raw_abi with host leafs: MulMat -> Add -> SoftMax"""
    rng_ = np.random.default_rng(3)
    K, M, N = 512, 300, 3
    w = (rng_.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
    x = rng_.standard_normal((N, K)).astype(np.float32)
    bias = rng_.standard_normal((N, M)).astype(np.float32)
    g = Graph()
    W, X, Bi = g.host(w, (K, M)), g.host(x, (K, N)), g.host(bias, (M, N))
    mm = g.node(R.MUL_MAT, (M, N), W, X)
    ad = g.node(R.ADD, (M, N), mm, Bi)
    g.inplace(R.SOFT_MAX, ad)
    z = x.astype(np.float64) @ w.astype(np.float64).T + bias
    z = np.exp(z - z.max(axis=1, keepdims=True))
    return g, z / z.sum(axis=1, keepdims=True)


def refused_cases():
    """[(name, Graph, index of the offending tensor, words the message must hold)]: one representative per hole; each is refused by lh_graph_check
    on the host.  Every graph starts with a well-formed strided MulMat (g_mul_mat, which the route trace records): a walk that began before the
    graph was refused would show there."""
    out = []
    x = np.arange(24, dtype=np.float32)

    def start(*extra):
        g = Graph()
        a, b = g.host(x, (4, 6)), g.host(x[::-1].copy(), (4, 6))
        more = [g.host(v) for v in extra]
        g.node(R.MUL_MAT, (6, 6), a, b)
        return [g, a, b] + more

    def done(name, g, words=None):
        bad = g.total - 1
        out.append((name, g, bad, words or f"tensor {bad}"))

    g, a, b = start(); g.node(R.ADD, (4, 6), a, b); g.t[-1].src0 = -2
    done("negative_source_index", g)
    g, a, b = start(); g.node(R.ADD, (4, 6), a, -1)
    done("missing_source", g)
    g, a, b = start(); g.node(R.MUL_MAT, (5, 6), a, b)          # declares 5 x 6, the kernel writes 6 x 6
    done("mul_mat_small_destination", g)
    g, a, b = start(); g.node(R.RMS_NORM, (4, 5), a)
    done("rms_norm_small_destination", g)
    g, a, b = start(); g.node(R.REPEAT, (6, 6), a)              # 6 is no multiple of 4
    done("repeat_not_a_multiple", g)
    g, a, b = start(); g.node(R.ADD, (4, 5), a, b)
    done("add_small_destination", g)
    g, a, b, p = start([np.nan]); g.inplace(R.DIAG_MASK_INF, a, p)
    done("diag_mask_past_nan", g)
    g, a, b, p = start([2]); g.inplace(R.DIAG_MASK_INF, a, p); g.t[-1].ne[1] = 5
    done("diag_mask_other_shape_than_its_source", g)
    g, a, b, ids = start([1, 2]); g.node(R.GET_ROWS, (3, 2), a, ids)
    done("get_rows_wrong_width", g)
    g, a, b, ids = start([1, 6]); g.node(R.GET_ROWS, (4, 2), a, ids)
    done("get_rows_id_past_the_table", g)
    # Add on a permuted 3-D operand: rows at j * ns1 leave the owner (hd = 4, N = 2, H = 3)
    g, a, b = start()
    pa = g.permute(g.view(a, (4, 3, 2), op=R.RESHAPE), (0, 2, 1, 3))      # ne = (4, 2, 3), ns = (1, 12, 4)
    g.node(R.ADD, (4, 2, 3), pa, g.view(b, (4, 2, 3), op=R.RESHAPE))
    done("add_permuted_rows_leave_owner", g)
    g, a, b = start()
    av = g.view(a, (2, 6))
    bv = g.view(b, (2, 6), nb=[8, 16, 96, 96])                # every second float of a row: nb10 != 4, the branch of ml.go:2567-2578
    g.node(R.ADD, (2, 6), av, bv)
    done("add_src1_not_contiguous", g, "src1")
    g, a, b = start(); g.node(R.ADD, (4, 6), a, b); g.t[-1].ne[2] = 0
    done("empty_extent", g)
    g, a, b = start(); g.node(R.ADD, (4, 6), a, b); g.t[-1].nb[1] = 18
    done("stride_not_whole_floats", g)
    g, a, b = start(); n = g.node(R.ADD, (4, 6), a, b); v = g.view(n, (4, 6)); g.t[v].view_off = 2 ** 64 - 1
    done("view_offset_wraps", g)
    for name, par in (("rope_past_nan", [np.nan, 4, 0]), ("rope_dims_2_pow_32", [0, 2.0 ** 32, 0])):
        g, a, b, p = start(par); g.inplace(R.ROPE, a, p)
        done(name, g)
    g, a, b, p = start([0, 2, 0]); pa = g.permute(a, (1, 0, 2, 3)); g.inplace(R.ROPE, pa, p)     # nb0 = 16: x[1] is no neighbour
    done("rope_pairs_not_adjacent", g)
    # counts the kernels keep in 32 bits; with zero strides such shapes fit any owner
    g, a, b = start(); v = g.view(a, (4, 2 ** 31), nb=[4, 0, 0, 0]); g.node(R.RMS_NORM, (4, 2 ** 31), v, nb=[4, 0, 0, 0])
    done("rms_norm_more_rows_than_a_launch_has_workgroups", g)
    g, a, b, p = start([2.0 ** 32 - 256]); v = g.view(a, (4, 300), nb=[4, 0, 0, 0]); g.inplace(R.DIAG_MASK_INF, v, p)
    done("diag_mask_past_plus_rows_wraps", g)
    # counts whose 32-bit sum wraps: to 0 (an empty graph would be LH_OK) and to the array's real length
    g, a, b = start(); g.counts = (2 ** 32 - 1, 1)
    done("counts_wrap_to_zero", g, "leafs + ")
    g, a, b = start(); g.counts = (2 ** 31 + g.n_leafs, 2 ** 31 + g.total - g.n_leafs)
    done("counts_wrap_to_the_array_length", g, "leafs + ")
    return out
