"""-m gpu: the gate of lh_graph_compute on a device - the same graph, on the same context, once with fusion allowed and once with
LH_GRAPH_NO_FUSION: whatever lh_last_graph_fused says, the two routes must agree.  The graphs are those of tests/test_graph_match_cpu.py (two
Eval graphs of `tiny`, the look-alikes of graph_match_cases.lookalikes, the regression mutants the matcher once fused wrongly), over weights
registered once per module.

A graph is sent to lh_graph_compute only after this test has asserted, on the host, that lh_graph_check accepts it - or that lh_graph_match
rejects it AND lh_graph_check refuses it, in which case the call must be refused before anything is launched (as tests/test_gpu_graph_refusal.py
does).  Per graph: seeded finite sentinels into both caches; compute with fusion allowed; read lh_last_graph_fused, the final node, both whole
caches; restore; compute node by node; read again; restore.  The final node and the cache rows the model (graph_ops_ref.run) says are written agree
within rel <= TOL of tests/test_gpu_llama.py; every other cache float keeps its sentinel's bits on both routes."""
import ctypes as C

import numpy as np
import pytest

import graph_match_cases as M
import graph_ops_ref as R
import node_path_abi as abi
import test_graph_check_cpu as GC
from llama_go_amd.mlapi import SHAPES

pytestmark = pytest.mark.gpu

TOL = M.TOL
BASES = (("tiny_N3_past0", 3, 0), ("tiny_N1_past5", 1, 5))
CTX = 64
LH_EUNSUPPORTED = R.LH_EUNSUPPORTED


class World:
    """one context, the weights of `tiny` registered once, the two base graphs bound to them"""

    def __init__(self, product):
        import llama_go_amd as pkg
        hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
        self.lib = abi.bind(hip)
        hip.lh_buf_upload.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, abi.F32P, C.c_uint64]
        hip.lh_buf_quantize_q8.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        hip.lh_last_graph_fused.argtypes = [C.c_void_p]
        self.match = M.Matching(hip)
        self.mirror = C.CDLL(pkg.LIBLLAMAGO)
        self.mirror.llamago_EvalGraphRecords.restype = C.c_int
        self.mirror.llamago_EvalGraphRecords.argtypes = [C.POINTER(GC.HParams), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(R.LhTensor), C.c_uint32, C.POINTER(C.c_uint32),
                                                         C.POINTER(R.LhBufExtent), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
        self.s = abi.Session(self.lib)
        self.bases, self.handle, self.inputs = {}, {}, {}
        for name, N, past in BASES:
            g = GC.eval_graph(self.mirror, "tiny", N, past, ctx=CTX)
            rc, info = self.match(g)
            assert rc == 1 and info == M.info_as_built(g, SHAPES["tiny"], N, past, CTX)
            inputs = M.seeded_inputs(g)
            for bid in sorted(g.bufs):                           # the mirror numbers the model's tensors alike in every graph of one shape
                if bid in self.inputs:
                    assert np.array_equal(self.inputs[bid], inputs[bid])
                else:
                    self.inputs[bid], self.handle[bid] = inputs[bid], self.s.register(inputs[bid])
            self.bases[name] = (g, info)

    def bound(self, g, handle=None):
        """a copy of g over the registered buffers"""
        handle = handle or self.handle
        h = g.copy()
        h.bufs = {handle[bid]: v for bid, v in g.bufs.items()}
        for t in h.t:
            if t.buf:
                t.buf = handle[t.buf]
        return h

    def upload(self, handle, data):
        data = np.ascontiguousarray(data, np.float32)
        assert self.lib.lh_buf_upload(self.s.ctx, handle, 0, data.ctypes.data_as(abi.F32P), data.size) == 0, self.s.error()

    def caches(self, g, info):
        """[(owner index, model buffer id)] of K and V"""
        return [(o, g.t[o].buf) for o in (info["kc_owner"], info["vc_owner"])]

    def one_route(self, h, flags, caches, handle, inputs):
        for o, bid in caches:
            self.upload(handle[bid], inputs[bid])
        rc, trace = abi.trace_of(self.lib, lambda: self.s.compute(h, flags))
        fused = self.lib.lh_last_graph_fused(self.s.ctx)
        final = None
        if rc == 0:
            last = h.t[h.total - 1]
            got, final = self.s.node_read(h.total - 1, last.ne[0] * last.ne[1])
            assert got == 0, self.s.error()
        mem = {o: self.s.read_buf(handle[bid], inputs[bid].size) for o, bid in caches}
        return rc, fused, final, mem, trace

    def both_routes(self, g, info, want_fused, handle=None, inputs=None):
        """g: a graph over MODEL buffer ids (info: where its caches are).  Returns the fused-allowed route's final node."""
        handle, inputs = handle or self.handle, inputs or self.inputs
        caches = self.caches(g, info)
        h = self.bound(g, handle)
        check = self.s.check(h)[0]
        verdict = self.match(h)[0]
        assert R.graph_fault(g) is None or check < 0
        if check != 0:
            # refused on the host: nothing may be launched, on either route, and the caches keep their bits
            assert check < 0 and verdict <= 0 and want_fused == 0, "neither accepted by lh_graph_check nor refused by both: not sent to the GPU"
            for flags in (0, abi.NO_FUSION):
                rc, fused, _, mem, trace = self.one_route(h, flags, caches, handle, inputs)
                assert rc == check and trace == [] and fused == 0, (rc, check, trace, self.s.error())
                for o, bid in caches:
                    assert np.array_equal(M.bits(mem[o]), M.bits(inputs[bid]))
            return None
        assert verdict == want_fused
        model = R.run(g, inputs)
        rc1, fused, final1, mem1, _ = self.one_route(h, 0, caches, handle, inputs)
        assert rc1 == 0, self.s.error()
        rc2, fused2, final2, mem2, _ = self.one_route(h, abi.NO_FUSION, caches, handle, inputs)
        assert rc2 == 0, self.s.error()
        for o, bid in caches:
            self.upload(handle[bid], inputs[bid])
        assert fused == want_fused and fused2 == 0, (fused, want_fused, fused2)
        err = M.rel(final1, final2)
        print(f"fused {fused}: final node rel {err:.3e}")
        assert err <= TOL, err
        assert any(model.written[o].any() for o, _ in caches)
        for o, bid in caches:
            w = model.written[o]
            if w.any():                                          # (K and V in one buffer: nothing lands in the other)
                err = M.rel(mem1[o][w], mem2[o][w])
                print(f"   cache {o}: {int(w.sum())} written floats rel {err:.3e}")
                assert err <= TOL, (o, err)
            for mem in (mem1, mem2):
                assert np.array_equal(M.bits(mem[o][~w]), M.bits(inputs[bid][~w])), f"cache {o}: floats outside the written rows changed"
        return final1

    def close(self):
        self.s.close()


@pytest.fixture(scope="module")
def world(product):
    w = World(product)
    yield w
    w.close()


@pytest.mark.parametrize("name", [b[0] for b in BASES])
def test_base_graphs_fuse_and_agree_with_the_node_path(world, name):
    g, info = world.bases[name]
    world.both_routes(g, info, 1)


@pytest.mark.parametrize("name", [b[0] for b in BASES])
def test_lookalikes_take_the_route_their_verdict_says_and_agree(world, name):
    g, info = world.bases[name]
    cases = M.lookalikes(g, info, world.inputs)
    assert len(cases) >= 12
    for case, h, _, verdict, want, why in cases:
        print(name, case)
        world.both_routes(h, want if verdict == 1 else info, 1 if verdict == 1 else 0)


def test_one_layer_model_on_a_cache_of_twice_the_size(world):
    g, shape, N, past, ctx = M.one_layer_graph(world.mirror)
    rc, info = world.match(g)
    assert rc == 1
    h = M.doubled(g, info)
    inputs = M.seeded_inputs(h, seed=77)
    s = world.s
    handle = {bid: s.register(inputs[bid]) for bid in sorted(h.bufs)}
    assert world.match(world.bound(h, handle))[1]["ctx"] == 2 * ctx
    world.both_routes(h, info, 1, handle, inputs)


@pytest.mark.parametrize("name", [b[0] for b in BASES])
def test_regression_mutants_run_node_by_node(world, name):
    """the mutants the matcher once fused although the sequential walk computes something else (chosen and measured by the model alone in
    tests/test_graph_match_cpu.py): fused == 0 now, and the call computes what the node path computes"""
    g, info = world.bases[name]
    arr, _, _ = g.pack()
    for mut in M.REGRESSION[name]:
        with GC.Mutated(g, arr, mut):
            h = g.copy()
        print(name, M.describe(g, mut))
        final = world.both_routes(h, info, 0)
        assert final is not None


def test_plans_follow_the_leafs_a_graph_names(world):
    """A, B (A with layer 0's wq bound to another buffer of the same shape), C (A over two other cache buffers), A again - on one context.  Every
    one fuses and equals its own node-path run: ModelDesc::same and the plan list tell them apart."""
    g, info = world.bases["tiny_N3_past0"]
    s = world.s
    wq = g.t[info["weights"][1]].buf
    other = (0.05 * np.random.default_rng(5).standard_normal(world.inputs[wq].size)).astype(np.float32)
    hb, ib = dict(world.handle), dict(world.inputs)
    hb[wq], ib[wq] = s.register(other), other
    hc, ic = dict(world.handle), dict(world.inputs)
    for o, bid in world.caches(g, info):
        ic[bid] = np.random.default_rng([9, bid]).uniform(-1, 1, world.inputs[bid].size).astype(np.float32)
        hc[bid] = s.register(ic[bid])
    a1 = world.both_routes(g, info, 1)
    b = world.both_routes(g, info, 1, hb, ib)
    c = world.both_routes(g, info, 1, hc, ic)
    a2 = world.both_routes(g, info, 1)
    assert M.rel(b, a1) > 100 * TOL, "B's weights do not move the result: the sequence proves nothing"
    assert M.rel(a2, a1) <= TOL
    assert M.rel(c, a1) <= TOL                                   # past = 0: the result does not depend on what the cache held


def test_block_int8_fuses_and_its_mutants_are_refused_on_the_host(world):
    """the same model after lh_buf_quantize_q8: the Eval graph fuses; the regression mutants cannot run anywhere - the node path has no dtype 7 -
    so they return LH_EUNSUPPORTED with nothing launched and the caches untouched, and the context then computes the Eval graph again"""
    name = "tiny_N1_past5"
    g, info = world.bases[name]
    s = world.s
    # the f32 graph is one lh_graph_check accepts; the block-int8 twin differs in the dtype of its matrices only (graph_match.h: exempt from that rule alone)
    assert s.check(world.bound(g))[0] == 0
    q = g.copy()
    handle = dict(world.handle)
    matrices = [w for k, w in enumerate(info["weights"]) if (k < 9 * info["L"] and k % 9 not in (0, 5)) or k == 9 * info["L"] + 2]
    for leaf in sorted(set(matrices)):
        t = q.t[leaf]
        out = C.c_uint64()
        assert world.lib.lh_buf_quantize_q8(s.ctx, world.handle[t.buf], t.ne[1], t.ne[0], C.byref(out)) == 0, s.error()
        s.bufs.append(out.value)
        handle[t.buf] = out.value
        t.dtype = 7
        q.bufs[t.buf] = (q.bufs[t.buf][0], 7)
    caches = world.caches(q, info)
    h = world.bound(q, handle)
    assert world.match(h) == (1, dict(info, wtype=7))

    def unmutated():
        rc, fused, final, mem, _ = world.one_route(h, 0, caches, handle, world.inputs)
        assert rc == 0, s.error()
        assert fused == 1 and np.isfinite(final).all()
        return final

    first = unmutated()
    arr, _, _ = q.pack()
    for mut in M.REGRESSION[name][:5]:
        with GC.Mutated(q, arr, mut):
            hm = world.bound(q, handle)
        assert world.match(hm)[0] == 0 and s.check(hm)[0] == LH_EUNSUPPORTED, "neither accepted by lh_graph_check nor refused by both: not sent to the GPU"
        rc, fused, _, mem, trace = world.one_route(hm, 0, caches, handle, world.inputs)
        assert rc == LH_EUNSUPPORTED and fused == 0 and trace == [], (rc, fused, trace, s.error())
        for o, bid in caches:
            assert np.array_equal(M.bits(mem[o]), M.bits(world.inputs[bid]))
    assert np.array_equal(M.bits(unmutated()), M.bits(first))
    for o, bid in caches:
        world.upload(handle[bid], world.inputs[bid])
