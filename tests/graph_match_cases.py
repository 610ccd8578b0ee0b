"""What tests/test_graph_match_cpu.py and tests/test_gpu_graph_match.py share: the binding of lh_graph_match (csrc/graph_match.h), the base Eval
graphs with their seeded data, the reference model of tests/graph_ops_ref.py run incrementally against a memoised base run, the look-alike
graphs one field cannot reach, and the regression list of mutants the matcher of the commit before this module fused although the sequential
walk computes something else.

The corpus, its mutation rule and the model are those of tests/test_graph_check_cpu.py (eval_graph, mutations, Mutated; graph_ops_ref.run,
graph_fault), imported, not restated."""
import ctypes as C

import numpy as np

import graph_ops_ref as R
import test_graph_check_cpu as GC

TOL = 1e-4                      # tests/test_gpu_llama.py


def rel(a, b):                  # tests/test_gpu_llama.py
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


class LhMatchInfo(C.Structure):  # struct lh_match_info (include/llamahip.h)
    _fields_ = [(k, C.c_uint32) for k in ("N", "past", "V", "d", "H", "hd", "L", "F", "ctx")] + \
               [(k, C.c_int32) for k in ("wtype", "kc_owner", "vc_owner", "tokens_leaf", "emb_node")] + \
               [("weights", C.POINTER(C.c_int32)), ("cap_weights", C.c_uint32), ("n_weights", C.c_uint32)]


SCALARS = ("N", "past", "V", "d", "H", "hd", "L", "F", "ctx", "wtype", "kc_owner", "vc_owner", "tokens_leaf", "emb_node")
W_NAMES = ("attention_norm", "wq", "wk", "wv", "wo", "ffn_norm", "w1", "w2", "w3")
CAP_WEIGHTS = 9 * 128 + 3


def bind(hip):
    hip.lh_graph_match.restype = C.c_int
    hip.lh_graph_match.argtypes = [C.POINTER(R.LhTensor), C.c_uint32, C.c_uint32, C.POINTER(R.LhBufExtent), C.c_uint32, C.POINTER(LhMatchInfo)]
    hip.lh_graph_check.restype = C.c_int
    hip.lh_graph_check.argtypes = [C.POINTER(R.LhTensor), C.c_uint32, C.c_uint32, C.POINTER(R.LhBufExtent), C.c_uint32, C.c_char_p, C.c_uint64]
    return hip


class Matching:
    """lh_graph_match with one output record kept across calls: (return code, info) where info is a dict (None unless accepted)"""

    def __init__(self, hip):
        self.hip = bind(hip)
        self.w = (C.c_int32 * CAP_WEIGHTS)()
        self.out = LhMatchInfo()

    def raw(self, arr, n_leafs, n_nodes, ext, nb):
        self.out.weights, self.out.cap_weights = self.w, CAP_WEIGHTS
        return self.hip.lh_graph_match(arr, n_leafs, n_nodes, ext, nb, C.byref(self.out))

    def info(self):
        o = self.out
        d = {k: getattr(o, k) for k in SCALARS}
        assert o.n_weights == 9 * o.L + 3 <= CAP_WEIGHTS
        d["weights"] = tuple(self.w[:o.n_weights])
        return d

    def __call__(self, g, packed=None):
        arr, ext, nb = packed or g.pack()
        rc = self.raw(arr, *g.abi_counts(), ext, nb)
        return rc, (self.info() if rc == 1 else None)


# ---- what the mirror built, read off the graph by its construction order (independent of the matcher) ---------------------------------------

def info_as_built(g, shape, N, past, ctx):
    """the lh_match_info of a mirror Eval graph from the hyper-parameters and from the order llama.Eval creates its tensors in (llama.go:239-384):
    within a layer the MulMats over weight leafs come as wq, wk (stored), wv (stored), wo, w1, w3 ... - told apart by their consumers"""
    d, H, L, V = shape["embd"], shape["heads"], shape["layers"], shape["vocab"]
    F = ((2 * (4 * d) // 3 + shape["mult"] - 1) // shape["mult"]) * shape["mult"]
    t = g.t
    users = {}
    for j, x in enumerate(t):
        for s in (x.src0, x.src1):
            if s >= 0:
                users.setdefault(s, []).append(j)
    mm = [j for j in range(g.n_leafs, g.total) if t[j].op == R.MUL_MAT and t[j].src0 < g.n_leafs and t[t[j].src0].buf]
    assert len(mm) == 7 * L + 1
    # the norm weights: under a Repeat, or - for N = 1, where ml.Repeat hands the leaf itself back (ml.go:487-513) - read by the Mul behind an RMSNorm
    gammas = [t[j].src0 if t[j].op == R.REPEAT else t[j].src0 for j in range(g.n_leafs, g.total)
              if t[j].op == R.REPEAT or (t[j].op == R.MUL and t[t[j].src1].op == R.RMS_NORM and t[j].src0 < g.n_leafs)]
    assert len(gammas) == 2 * L + 1
    w = []
    caches = []
    for il in range(L):
        by = {}                                                  # the seven MulMats over weights of the layer, told apart by their consumers
        for j in mm[7 * il:7 * il + 7]:
            u = t[users[j][0]]
            if u.op == R.CPY and t[u.src1].op == R.VIEW:
                by.setdefault("store", []).append(j)
            elif u.op == R.CPY:
                by["q"] = j
            elif u.op == R.SILU:
                by["w1"] = j
            elif u.op == R.MUL:
                by["w3"] = j
            elif u.op == R.ADD and t[t[j].src1].op == R.CPY:
                by["o"] = j
            else:
                by["w2"] = j
        own = {t[t[users[s][0]].src1].storage: s for s in by["store"]}
        kc = next(t[j].storage for j in range(g.n_leafs, g.total) if t[j].op == R.ROPE and t[t[j].storage].buf)   # K is the cache that is rotated
        vc = next(o for o in own if o != kc)
        sk, sv = own[kc], own[vc]
        caches.append((kc, vc))
        w += [gammas[2 * il], t[by["q"]].src0, t[sk].src0, t[sv].src0, t[by["o"]].src0, gammas[2 * il + 1], t[by["w1"]].src0, t[by["w2"]].src0, t[by["w3"]].src0]
    assert len(set(caches)) == 1
    get_rows = next(j for j in range(g.n_leafs, g.total) if t[j].op == R.GET_ROWS)
    w += [t[get_rows].src0, gammas[2 * L], t[mm[-1]].src0]
    return dict(N=N, past=past, V=V, d=d, H=H, hd=d // H, L=L, F=F, ctx=ctx, wtype=0, kc_owner=caches[0][0], vc_owner=caches[0][1],
                tokens_leaf=t[get_rows].src1, emb_node=t[g.total - 1].src1, weights=tuple(w))


# ---- seeded data ------------------------------------------------------------------------------------------------------------------------------

def seeded_inputs(g, seed=20240):
    """{buffer id: fp32 array}: Gaussian weights (matrices and embeddings N(0, 0.05^2), norm vectors N(1, 0.1^2)) and caches of seeded finite values"""
    out = {}
    for i, t in enumerate(g.t[:g.n_leafs]):
        if not t.buf:
            continue
        r = np.random.default_rng([seed, t.buf])
        n = g.bufs[t.buf][0]
        if any(u.storage == i and u is not t for u in g.t):
            out[t.buf] = r.uniform(-1, 1, n).astype(np.float32)                           # a cache: views lie in it
        elif t.ne[1] == 1:
            out[t.buf] = (1 + 0.1 * r.standard_normal(n)).astype(np.float32)              # a norm vector (under a Repeat, or read by the Mul itself when N = 1)
        else:
            out[t.buf] = (0.05 * r.standard_normal(n)).astype(np.float32)
    return out


# ---- the model, incrementally -------------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_result(a, b):
    if a is None or b is None:
        return a is b
    return a.owner == b.owner and a.offs.shape == b.offs.shape and np.array_equal(a.offs, b.offs) and np.array_equal(bits(a.y32), bits(b.y32))


class BaseRun:
    """graph_ops_ref.run of the unmutated graph, memoised: every node's result, and the state of every owner in front of every node"""

    def __init__(self, g, inputs):
        self.g, self.inputs = g.copy(), inputs                   # (Mutated changes the caller's graph in place, host values included)
        g = self.g
        self.run = R.run(g, inputs)
        self.writers = {}
        for j in sorted(self.run.nodes):
            self.writers.setdefault(self.run.nodes[j].owner, []).append(j)
        self._initial = {}
        self.final = self.run.nodes[g.total - 1]
        self.buffers = [i for i, t in enumerate(g.t) if t.storage == i and t.buf]

    def initial(self, g, o, memo=True):
        if memo and o in self._initial:
            return self._initial[o]
        t = g.t[o]
        n = R.owner_size(g, o)
        a = np.asarray(self.inputs[t.buf], np.float32).reshape(-1) if t.buf else t.host[:n].copy() if t.host is not None else R.sentinel(n)
        if memo:
            self._initial[o] = a
        return a

    def state(self, o, j):
        """owner o of the BASE graph in front of node j (read-only: may be the memoised array itself)"""
        ws = self.writers.get(o, ())
        if not ws or ws[0] >= j:
            return self.initial(self.g, o)
        if ws[-1] < j:
            return self.run.mem[o]
        a = self.initial(self.g, o).copy()
        for w in ws:
            if w >= j:
                break
            a[self.run.nodes[w].offs] = self.run.nodes[w].y32
        return a

    def mutant(self, g, i, trace=None):
        """Run the mutant g (tensor i differs from the base graph; the model calls g safe) from the first node the change can reach.  A node is
        executed again when tensor i is the node itself, one of its sources, or the owner of its storage, or when it touches an owner whose
        contents differ from the base run's at that point; every other node keeps its memoised result.  Returns (identical, final node's result,
        {buffer owner: final contents} of the buffers that were touched): identical means the final node's values and offsets and every float
        of every registered buffer carry the base run's bits.  trace (a list): receives (node, result) of every node that was executed again."""
        t = g.t
        direct = {j for j in range(g.n_leafs, g.total) if j == i or t[j].src0 == i or t[j].src1 == i or t[j].storage == i}
        over = {}
        if t[i].storage == i:
            now = self.initial(g, i, memo=False)
            before = self.initial(self.g, i) if self.g.t[i].storage == i else None
            if before is None or now.shape != before.shape or not np.array_equal(bits(now), bits(before)):
                over[i] = np.array(now, dtype=np.float32)
        first = min(direct) if direct else g.total
        if over:
            first = g.n_leafs
        base = self

        class Mem:
            def __init__(self):
                self.j = 0

            def __getitem__(self, o):
                return over[o] if o in over else base.state(o, self.j)

        mem = Mem()
        final = self.final
        for j in range(first, g.total):
            x = t[j]
            if x.op not in R.ARITY or R.ARITY[x.op] == 0:
                if j in self.run.nodes and j in direct:          # the node no longer runs: what it wrote stays as it was in front of it
                    o = self.run.nodes[j].owner
                    if o not in over:
                        over[o] = np.array(self.state(o, j))
                continue
            touched = {x.storage, t[x.src0].storage} | ({t[x.src1].storage} if R.ARITY[x.op] == 2 else set())
            if j not in direct and not (touched & over.keys()):
                continue
            mem.j = j
            res = R.exec_node(g, j, mem)
            if trace is not None:
                trace.append((j, res))
            was = self.run.nodes.get(j)
            if res.owner not in over:
                if same_result(res, was):
                    continue
                over[res.owner] = np.array(self.state(res.owner, j))     # (an owner the mutation made or resized is in `over` from the start)
            if was is not None and was.owner != res.owner and was.owner not in over:
                over[was.owner] = np.array(self.state(was.owner, j))     # the base run wrote there, this one does not
            over[res.owner][res.offs] = res.y32
            if j == g.total - 1:
                final = res
        bufs = {o: a for o, a in over.items() if t[o].storage == o and t[o].buf}
        identical = same_result(final, self.final) and all(o in self.run.mem and a.shape == self.run.mem[o].shape and np.array_equal(bits(a), bits(self.run.mem[o]))
                                                           for o, a in bufs.items())
        return identical, final, bufs


# ---- look-alikes one field cannot reach -------------------------------------------------------------------------------------------------------

def find(g, op, nth=0, pred=lambda t: True):
    return [j for j in range(g.n_leafs, g.total) if g.t[j].op == op and pred(g.t[j])][nth]


def renumber(g, order):
    """the graph with its tensors in `order` (a permutation of range(total); leafs stay first)"""
    new = {old: k for k, old in enumerate(order)}
    h = g.copy()
    h.t = [g.t[old].copy() for old in order]
    for t in h.t:
        t.src0 = new[t.src0] if t.src0 >= 0 else -1
        t.src1 = new[t.src1] if t.src1 >= 0 else -1
        t.storage = new[t.storage]
    return h


def layer_nodes(g, info, il):
    """indices of layer il's attention by role, read off the base graph through the wiring (as the sequential walk would see them)"""
    t = g.t
    W = info["weights"][9 * il:9 * il + 9]
    mm = lambda leaf: next(j for j in range(g.n_leafs, g.total) if t[j].op == R.MUL_MAT and t[j].src0 == leaf)
    user = lambda j, op: next(u for u in range(g.n_leafs, g.total) if t[u].op == op and (t[u].src0 == j or t[u].src1 == j))
    mq, mk, mv = mm(W[1]), mm(W[2]), mm(W[3])
    ks, vs = user(mk, R.CPY), user(mv, R.CPY)
    qc = user(mq, R.CPY)
    qr = user(qc, R.ROPE)
    kq = user(user(qr, R.PERMUTE), R.MUL_MAT)
    kr = t[t[kq].src0].src0
    sc = user(kq, R.SCALE)
    dm = user(sc, R.DIAG_MASK_INF)
    sm = user(dm, R.SOFT_MAX)
    kqv = user(sm, R.MUL_MAT)
    return dict(mq=mq, mk=mk, mv=mv, kstore=ks, vstore=vs, kview=t[ks].src1, vview=t[vs].src1, qc=qc, qr=qr, kr=kr, kq=kq, scale=sc, mask=dm, soft=sm, kqv=kqv,
                vt=t[kqv].src0)


def with_leafs(g, n_new):
    """room for n_new leafs in front of the nodes: (copy of g with every index shifted, index of the first new leaf)"""
    h = g.copy()
    at = g.n_leafs
    sh = lambda k: k + n_new if k >= at else k
    for t in h.t:
        t.src0, t.src1, t.storage = (sh(t.src0) if t.src0 >= 0 else -1), (sh(t.src1) if t.src1 >= 0 else -1), sh(t.storage)
    for k in range(n_new):
        x = R.T(R.NONE, [1, 1, 1, 1], [4, 4, 4, 4], storage=at + k)
        h.t.insert(at + k, x)
    h.n_leafs += n_new
    return h, at, sh


def host_leaf(h, i, values):
    v = np.asarray(values, np.float32)
    h.t[i] = R.T(R.NONE, [v.size, 1, 1, 1], R.packed_nb([v.size, 1, 1, 1]), storage=i, host=v)


def lookalikes(g, info, inputs):
    """[(name, graph, inputs, verdict, expected info or None, why)] built from the base graph g (its lh_match_info: info) by small edits.
    verdict 0: the matcher must reject - the sequential walk of the graph does not compute what the fused plan of the base would; 1: must accept,
    with the stated info - the graph is an Eval over other leafs."""
    out = []
    L0 = layer_nodes(g, info, 0)
    t = g.t
    total = g.total
    d, N, past, ctx = info["d"], info["N"], info["past"], info["ctx"]

    # -- rejected
    order = list(range(total))
    for s in sorted((L0["kstore"], L0["vstore"])):               # the two store Cpys move behind the layer's last attention node
        order.remove(s)
    at = order.index(L0["kqv"]) + 1
    order[at:at] = [L0["kstore"], L0["vstore"]]
    out.append(("stores_behind_attention", renumber(g, order), inputs, 0, None,
                "the attention of layer 0 reads the cache rows before the stores write them: stale rows"))

    h = g.copy()
    extra = h.node(R.SILU, h.t[L0["mq"]].ne, L0["mq"])           # reads an intermediate; appended, then moved in front of the final node
    order = list(range(total - 1)) + [extra, total - 1]
    out.append(("extra_reader_of_an_intermediate", renumber(h, order), inputs, 0, None, "a node outside the pattern: every node must be claimed"))

    h = g.copy()
    kv = h.t[L0["kview"]]
    v2 = h.node(R.VIEW, kv.ne, kv.src0, -1, nb=list(kv.nb), like=L0["kview"])
    c2 = h.node(R.CPY, kv.ne, L0["mv"], v2, nb=list(kv.nb), like=v2)  # wv . h1 lands on the K rows a second time
    order = list(range(total))
    at = order.index(max(L0["kstore"], L0["vstore"])) + 1        # behind both stores (wv . h1 exists there), in front of the attention
    order[at:at] = [v2, c2]
    out.append(("second_k_store_into_the_same_rows", renumber(h, order), inputs, 0, None, "the later store wins in the sequential walk"))

    h = g.copy()
    sc = h.t[h.t[L0["scale"]].src1]
    sc.host = (sc.host.astype(np.float64) * (1 + 2.0 ** -23)).astype(np.float32)
    assert sc.host[0] != g.t[g.t[L0["scale"]].src1].host[0]
    out.append(("scale_one_ulp_off", h, inputs, 0, None, "the plan scales by 1/sqrt(hd) exactly"))

    h = g.copy()
    h.t[L0["kr"]].src1, h.t[L0["qr"]].src1 = g.t[L0["qr"]].src1, g.t[L0["kr"]].src1
    out.append(("rope_modes_exchanged", h, inputs, 0, None, "K would be rotated from position `past` on and Q as a cache"))

    h = g.copy()
    pl = h.t[h.t[L0["mask"]].src1]
    pl.host = np.asarray([past + 1], np.float32)
    out.append(("mask_past_differs_from_rope_past", h, inputs, 0, None, "the plan masks with the Rope's `past`"))

    if info["L"] > 1:
        L1 = layer_nodes(g, info, 1)
        h = g.copy()
        shift = ctx * d
        for j in range(h.n_leafs, total):
            x = h.t[j]
            if x.storage in (info["kc_owner"], info["vc_owner"]) and x.view_off >= shift:
                x.view_off -= shift
        out.append(("two_layers_on_one_cache_slot", h, inputs, 0, None, "layer 1 overwrites the rows layer 0 of the next Eval reads"))
        del L1

    h = g.copy()
    for j, x in enumerate(h.t):
        if x.storage == info["vc_owner"]:
            x.storage = info["kc_owner"]
    h.t[info["vc_owner"]].storage = info["vc_owner"]
    out.append(("k_and_v_in_one_buffer", h, inputs, 0, None, "the V store overwrites the K rows"))

    h = g.copy()
    ids = h.t[info["tokens_leaf"]]
    if N > 1:
        ids.ne[0], ids.host = N - 1, ids.host[:N - 1].copy()
        ids.nb = R.packed_nb(ids.ne)
    else:                                                        # N = 1: the leaf cannot be shorter than one id; an empty extent is a structural refusal
        ids.ne[0] = 0
    out.append(("token_leaf_shorter_than_n", h, inputs, 0 if N > 1 else R.LH_ESHAPE, None, "GetRows would read ids the caller never gave"))

    h = g.copy()
    wq = h.t[info["weights"][1]]
    wq.nb[1] += 4                                               # rows one float apart from packed: the leaf is a strided window, no plain matrix
    out.append(("weight_leaf_not_contiguous", h, inputs, 0, None, "the plan streams weights as packed matrices"))

    # -- accepted
    if info["L"] > 1:
        h = g.copy()
        mq = h.t[L0["mq"]]
        mq.src0 = info["weights"][9 + 1]
        w = list(info["weights"])
        w[1] = w[9 + 1]
        out.append(("layer0_uses_layer1_wq", h, inputs, 1, dict(info, weights=tuple(w)), "an Eval over another weight leaf"))

    h = g.copy()
    swap = {info["kc_owner"]: info["vc_owner"], info["vc_owner"]: info["kc_owner"]}
    for x in h.t[h.n_leafs:]:
        x.storage = swap.get(x.storage, x.storage)
        if x.op == R.VIEW:
            x.src0 = swap.get(x.src0, x.src0)
    out.append(("cache_owners_exchanged", h, inputs, 1, dict(info, kc_owner=info["vc_owner"], vc_owner=info["kc_owner"]), "an Eval over the two caches the other way round"))

    h = g.copy()
    ids = h.t[info["tokens_leaf"]]
    ids.host = np.asarray([(7 * k + 3) % info["V"] for k in range(N)], np.float32)
    out.append(("other_token_ids", h, inputs, 1, dict(info), "an Eval of other tokens"))
    return out


def eval_graph_of(mirror, shape, N, past, ctx):
    """GC.eval_graph for a shape given as a dict (GC.eval_graph looks its argument up in mlapi.SHAPES)"""
    from llama_go_amd.mlapi import SHAPES
    SHAPES["_graph_match"] = shape
    try:
        return GC.eval_graph(mirror, "_graph_match", N, past, ctx=ctx)
    finally:
        del SHAPES["_graph_match"]


def one_layer_graph(mirror):
    """a one-layer model (see doubled): (graph, shape, N, past, ctx)"""
    from llama_go_amd.mlapi import SHAPES
    shape = dict(SHAPES["tiny"], layers=1)
    return eval_graph_of(mirror, shape, 3, 2, 32), shape, 3, 2, 32


def doubled(g, info):
    """cache buffers of twice the size under a one-layer graph: the matcher reads ctx off the buffer (embd * layers * ctx floats), so ctx doubles -
    and with one layer every offset of the graph stays what an Eval at that ctx would have built"""
    h = g.copy()
    for o in (info["kc_owner"], info["vc_owner"]):
        x = h.t[o]
        n = h.bufs[x.buf][0]
        h.bufs[x.buf] = (2 * n, 0)
        x.ne[0] = 2 * n
        x.nb = R.packed_nb(x.ne)
    return h


# ---- single-field mutants ---------------------------------------------------------------------------------------------------------------------

def kind_of(f):
    if R.F_NE <= f < R.F_NE + 4:
        return "ne"
    if R.F_NB <= f < R.F_NB + 4:
        return "nb"
    return {R.F_VIEW_OFF: "view_off", R.F_STORAGE: "storage", R.F_OP: "op", R.F_SRC0: "src", R.F_SRC1: "src", R.F_SWAP: "src", R.F_FLAGS: "flags",
            R.F_HOST_VALUE: "host", R.F_HOST_NULL: "host", R.F_COUNTS: "counts", R.F_NONE: "none"}[f]


def unit_stride_family(g, mut):
    """(tensor, dimension) when the mutation sets the stride of a dimension of extent 1 to one of the ~50 values mutations() lists for it, else None"""
    i, f, v = mut
    if not (R.F_NB <= f < R.F_NB + 4):
        return None
    k = f - R.F_NB
    t = g.t[i]
    if t.ne[k] != 1 or v % 4 or v == 0 or v >= 2 ** 63 or v == t.nb[k]:
        return None
    return (i, k)


def family_representatives(g, muts):
    """{(tensor, dimension): the three values of the family the model is run for: the smallest, 3 x the original stride, the largest}"""
    fam = {}
    for mut in muts:
        key = unit_stride_family(g, mut)
        if key is not None:
            fam.setdefault(key, []).append(mut[2])
    return {key: {min(vs), 3 * g.t[key[0]].nb[key[1]], max(vs)} for key, vs in fam.items()}


MAX_MODELLED_OWNER = 2 ** 26   # floats


class Row:
    __slots__ = ("mut", "kind", "rc", "info", "check", "fault", "identical", "family")


def survey(match, g, inputs, base=None):
    """Every single-field mutant of g (GC.mutations): the matcher's verdict for ALL of them, the model's for all but the thinned unit-stride
    families.  Row.identical: True / False from the model's run (BaseRun.mutant), None where the model calls the mutant unsafe (Row.fault) or the
    mutant is a family member the model is not run for.  Declared identical without a run: F_NONE and the flags mutants only - the model has no
    notion of flags (no op_reach rule, no line of exec_node reads them), so every address and every value is unchanged."""
    base = base or BaseRun(g, inputs)
    muts = GC.mutations(g)
    reps = family_representatives(g, muts)
    arr, ext, nb = g.pack()
    assert R.graph_fault(g) is None
    rows = []
    for mut in muts:
        r = Row()
        r.mut, r.kind, r.family = mut, kind_of(mut[1]), unit_stride_family(g, mut)
        with GC.Mutated(g, arr, mut) as m:
            r.rc = match.raw(arr, m.counts[0], m.counts[1], ext, nb)
            r.info = match.info() if r.rc == 1 else None
            r.check = match.hip.lh_graph_check(arr, m.counts[0], m.counts[1], ext, nb, None, 0) if r.rc == 1 else None
            if mut[1] == R.F_COUNTS:
                r.fault = R.graph_fault(g, m.counts[0], m.counts[1])
            else:
                r.fault = R.graph_fault(g, only=R.dependents(g, mut[0]) | GC.self_before(m))
            if r.fault is not None:
                r.identical = None
            elif r.kind in ("none", "flags"):
                r.identical = True
            elif r.family is not None and mut[2] not in reps[r.family]:
                r.identical = None
            elif g.t[mut[0]].storage == mut[0] and R.owner_size(g, mut[0]) > MAX_MODELLED_OWNER:
                r.identical = None                               # (safe by the model's rules, too large to allocate: never accepted, asserted by the test)
            else:
                r.identical = base.mutant(g, mut[0])[0]
        rows.append(r)
    return rows


def describe(g, mut):
    i, f, v = mut
    name = {R.F_OP: "op", R.F_SRC0: "src0", R.F_SRC1: "src1", R.F_STORAGE: "storage", R.F_VIEW_OFF: "view_off", R.F_HOST_NULL: "host=NULL", R.F_COUNTS: "counts",
            R.F_FLAGS: "flags", R.F_SWAP: "src0<->src1", R.F_NONE: "nothing"}.get(f)
    if name is None:
        name = f"ne[{f - R.F_NE}]" if R.F_NE <= f < R.F_NE + 4 else f"nb[{f - R.F_NB}]" if R.F_NB <= f < R.F_NB + 4 else f"host[{v >> 32}] bits"
        if f == R.F_HOST_VALUE:
            v = hex(v & 0xffffffff)
    t = g.t[i]
    return f"tensor {i} (op {t.op}, ne {t.ne}): {name} = {v}"


def margin(base, final, bufs):
    """how far a mutant's run (BaseRun.mutant) lies from the base run: the larger of rel() over the final node and over the rows of each touched
    cache the base run writes; inf where the shapes differ or a value is no number"""
    a, b = final.y32, base.final.y32
    if a.shape != b.shape:
        return float("inf")
    worst = [rel(a, b)]
    for o, arr in bufs.items():
        w = base.run.written[o]
        if w.any():
            worst.append(rel(arr[w], base.run.mem[o][w]))
    return float("inf") if any(x != x for x in worst) else max(worst)


# Mutants of the two base graphs of tests/test_graph_match_cpu.py (tensor, field, value) that the matcher of the commit before this file accepted
# although the model calls them safe and computes something else - by the margin in the comment (margin(): rel() to the base run), at least 100 x TOL.
# Chosen from that matcher's false positives (profiles/matcher_mutants.txt), at most three per (field, op), among those a device can repeat: the
# margin is finite (the run reads no float that nothing wrote) and no node writes one address twice - the sequential walk lets the last write
# win, kernels that write in parallel cannot, so two device runs of such a graph need not agree (strides of 0 or below the row on a destination;
# the node path accepts them).
REGRESSION = {
    "tiny_N3_past0": [
        (44, 13, 1),      # the K store Cpy [768]: view_off = 1: 1.47
        (44, 13, 2),      # the K store Cpy: view_off = 2: 1.32
        (44, 13, 5),      # the K store Cpy: view_off = 5: 1.24
        (50, 13, 1),      # Permute of the V cache view [3, 64, 4]: view_off = 1: 1.49
        (50, 13, 2),      # Permute of the V cache view: view_off = 2: 1.22
        (50, 13, 5),      # Permute of the V cache view: view_off = 5: 1.5
        (53, 11, 1028),   # Reshape3D of the K cache view [64, 4, 3], layer 0: nb[2] = 1028: 1.04
        (92, 11, 1028),   # Reshape3D of the K cache view, layer 1: nb[2] = 1028: 0.745
    ],
    "tiny_N1_past5": [
        (43, 13, 0),      # the K store Cpy [256]: view_off = 0: 1.24
        (43, 13, 1),      # the K store Cpy: view_off = 1: 1.24
        (43, 13, 2),      # the K store Cpy: view_off = 2: 1.24
        (49, 13, 1),      # Permute of the V cache view [6, 64, 4]: view_off = 1: 1.4
        (49, 13, 2),      # Permute of the V cache view: view_off = 2: 1.43
        (49, 13, 5),      # Permute of the V cache view: view_off = 5: 1.56
        (52, 10, 260),    # Reshape3D of the K cache view [64, 4, 6], layer 0: nb[1] = 260: 1.34
        (52, 11, 0),      # Reshape3D of the K cache view: nb[2] = 0 (the Rope of mode 1 turns one position only): 1.05
        (52, 11, 1020),   # Reshape3D of the K cache view: nb[2] = 1020: 1.15
        (52, 11, 1028),   # Reshape3D of the K cache view: nb[2] = 1028: 1.36
        (89, 10, 260),    # Reshape3D of the K cache view, layer 1: nb[1] = 260: 0.966
    ],
}
