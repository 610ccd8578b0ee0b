"""not-gpu: lh_graph_match (csrc/graph_match.h) - the gate that decides whether lh_graph_compute runs a graph as the fused LLaMA plan - held to
the result of the reference's sequential walk, without a device.  The fused result is a function of lh_match_info and of the data alone, so a
graph may be accepted only if the model of the node path (tests/graph_ops_ref.py) computes, for it, what it computes for the Eval graph with
that lh_match_info.

  soundness      every single-field mutant (the corpus of tests/test_graph_check_cpu.py: mutations, Mutated) of two Eval graphs that the matcher
                 ACCEPTS is safe by the model (graph_fault is None), carries the unmutated graph's lh_match_info, is accepted by lh_graph_check,
                 and the model's run of it equals the run of the unmutated graph bit for bit: the final node and every float of every
                 registered buffer.  The matcher's verdict is taken for every mutant; the model runs incrementally against a memoised base run
                 (graph_match_cases.BaseRun) for every safe mutant except: flags (the model has no notion of them) and, of the ~50 strides
                 tried on a dimension of extent 1, all but three per (tensor, dimension) - for which the matcher must give the whole family one
                 verdict.
  completeness   every Eval graph of the mirror over three shapes, seven N and four `past` is accepted with the lh_match_info it was built with.
  look-alikes    graphs one field cannot reach, each with the verdict it must get and why (graph_match_cases.lookalikes).
  regression     mutants the matcher of the commit before this file fused although the walk computes something else by at least 100 x the
                 suite's tolerance: chosen and checked by the model alone; tests/test_gpu_graph_match.py sends them to a device.

profiles/matcher_mutants.txt holds the report of this module for the matcher before and after the fix."""
import ctypes as C
import time

import numpy as np
import pytest

import graph_match_cases as M
import graph_ops_ref as R
import test_graph_check_cpu as GC
from llama_go_amd.mlapi import SHAPES

BASES = (("tiny_N3_past0", 3, 0), ("tiny_N1_past5", 1, 5))
CTX = 64


@pytest.fixture(scope="module")
def hip(built):
    import llama_go_amd as pkg
    return C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)


@pytest.fixture(scope="module")
def mirror(hip):
    import llama_go_amd as pkg
    m = C.CDLL(pkg.LIBLLAMAGO)
    m.llamago_EvalGraphRecords.restype = C.c_int
    m.llamago_EvalGraphRecords.argtypes = [C.POINTER(GC.HParams), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(R.LhTensor), C.c_uint32, C.POINTER(C.c_uint32),
                                           C.POINTER(R.LhBufExtent), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    return m


@pytest.fixture(scope="module")
def match(hip):
    return M.Matching(hip)


@pytest.fixture(scope="module")
def bases(mirror, match):
    out = {}
    for name, N, past in BASES:
        g = GC.eval_graph(mirror, "tiny", N, past, ctx=CTX)
        rc, info = match(g)
        assert rc == 1, f"{name}: the unmutated Eval graph is not accepted"
        assert info == M.info_as_built(g, SHAPES["tiny"], N, past, CTX)
        inputs = M.seeded_inputs(g)
        out[name] = (g, info, inputs, M.BaseRun(g, inputs))
    return out


@pytest.fixture(scope="module")
def surveys(bases, match):
    out = {}
    for name, (g, info, inputs, base) in bases.items():
        t0 = time.perf_counter()
        out[name] = (M.survey(match, g, inputs, base), time.perf_counter() - t0)
    return out


def false_positives(rows, info):
    return [r for r in rows if r.rc == 1 and (r.fault is not None or r.identical is False or r.info != info or r.check != 0)]


def test_soundness_every_accepted_mutant_is_the_base_graph_to_the_sequential_walk(bases, surveys):
    report = []
    for name, (g, info, inputs, base) in bases.items():
        rows, seconds = surveys[name]
        assert all(r.rc in (0, 1) or r.rc < 0 for r in rows)
        accepted = [r for r in rows if r.rc == 1]
        fp = false_positives(rows, info)
        ran = sum(r.identical is not None and r.kind not in ("flags", "none") for r in rows)
        report.append(f"{name}: {len(rows)} mutants, {len(accepted)} accepted, {sum(r.identical is True for r in accepted)} of those identical by the model's run "
                      f"(the others: members of unit-stride families whose three representatives are), {len(fp)} false positives; "
                      f"model runs {ran}, {seconds:.1f} s")
        print(report[-1])
        for r in fp[:10]:
            print("   false positive:", M.describe(g, r.mut), "| model:", r.fault or ("identical" if r.identical else "another result"), "| lh_graph_check", r.check,
                  "| info differs" if r.info != info else "")
        assert not fp, f"{name}: {len(fp)} false positives, first: {M.describe(g, fp[0].mut)}"
        # an accepted mutant the model was not run for is a member of a unit-stride family (next test: one verdict per family, so its
        # representatives were accepted, run and found identical above)
        for r in accepted:
            assert r.identical is True or (r.fault is None and r.family is not None), M.describe(g, r.mut)
        assert len(accepted) > 100, "the matcher accepts (nearly) nothing: soundness is vacuous"


def test_unit_stride_families_get_one_verdict(bases, surveys):
    for name, (g, info, inputs, base) in bases.items():
        fam = {}
        for r in surveys[name][0]:
            if r.family is not None:
                fam.setdefault(r.family, []).append(r)
        assert len(fam) > 100
        for key, rs in fam.items():
            assert len(rs) >= 40, (key, len(rs))
            assert len({r.rc for r in rs}) == 1, f"{name}: tensor {key[0]} nb[{key[1]}]: verdicts {sorted({r.rc for r in rs})} within one family"
            assert sum(r.identical is not None or r.fault is not None for r in rs) >= 3


def test_the_corpus_means_something(bases, surveys):
    """by the model alone: every kind of field has mutants that are the base graph to the sequential walk (identical run) and mutants that are not
    (another result, or a graph the walk halts or faults on).  `flags` cannot have the second sort - the model, like the node path, materialises
    every node whatever its flags - and a storage index can only name another valid owner where the tensor is the corpus' `view` itself."""
    both = {}
    for name, (g, info, inputs, base) in bases.items():
        kinds = {}
        for r in surveys[name][0]:
            sort = "identical" if r.identical is True else "another_result" if r.identical is False else "unsafe" if r.fault is not None else "not_run"
            for table in (kinds, both):
                k = table.setdefault(r.kind, dict(identical=0, another_result=0, unsafe=0, not_run=0))
                k[sort] += 1
        print(name, {k: tuple(v.values()) for k, v in kinds.items()}, "(identical, another result, unsafe, not run)")
        for k in ("ne", "nb", "view_off", "op", "src", "host"):
            assert kinds[k]["identical"] > 0 and kinds[k]["another_result"] + kinds[k]["unsafe"] > 0, (name, k, kinds[k])
        for k in ("nb", "view_off", "op", "src", "host"):
            assert kinds[k]["another_result"] > 0, (name, k, kinds[k])
        assert kinds["flags"]["identical"] > 0 and kinds["flags"]["another_result"] == kinds["flags"]["unsafe"] == 0
        assert kinds["counts"]["unsafe"] == 6
    # (at past > 0 the corpus' `view` lies at an offset no owner of its size has: there the one valid storage mutant is unsafe too)
    assert both["storage"]["identical"] > 0 and both["storage"]["unsafe"] > 0, both["storage"]


COMPLETE_CTX = 160


@pytest.mark.parametrize("shape", ["tiny", "small", "hd128"])
def test_completeness_every_eval_graph_of_the_mirror_is_accepted_as_built(mirror, match, shape):
    if shape == "hd128":
        from test_gpu_batch_feed import HD128 as hp               # 5 heads of 128 (importing a gpu module runs none of its tests)
    else:
        hp = SHAPES[shape]
    count = 0
    for N in (1, 2, 3, 8, 9, 33, 129):
        for past in (0, 1, 5, COMPLETE_CTX - N):
            g = M.eval_graph_of(mirror, hp, N, past, COMPLETE_CTX)
            rc, info = match(g)
            assert rc == 1, (shape, N, past)
            assert info == M.info_as_built(g, hp, N, past, COMPLETE_CTX), (shape, N, past)
            assert GC.check(match.hip, g)[0] == 0
            count += 1
    assert count == 28


def test_lookalikes_get_the_stated_verdict(bases, match, mirror):
    seen = 0
    for name, (g, info, inputs, base) in bases.items():
        for case, h, _, verdict, want, why in M.lookalikes(g, info, inputs):
            rc, got = match(h)
            assert rc == verdict, f"{name} / {case}: verdict {rc}, must be {verdict}: {why}"
            if verdict == 1:
                assert got == want, (name, case)
                assert R.graph_fault(h) is None and GC.check(match.hip, h)[0] == 0, (name, case)
            seen += 1
    assert seen >= 2 * 12
    # a cache buffer of twice the size on a one-layer model: ctx doubles, everything else stays
    g, shape, N, past, ctx = M.one_layer_graph(mirror)
    rc, info = match(g)
    assert rc == 1 and info == M.info_as_built(g, shape, N, past, ctx)
    h = M.doubled(g, info)
    rc, got = match(h)
    assert rc == 1 and got == dict(info, ctx=2 * ctx)
    assert R.graph_fault(h) is None
    # ... and on the two-layer base the same edit moves nothing in the graph, so layer 1 no longer lies at its slot: rejected
    g, info = bases["tiny_N3_past0"][:2]
    assert match(M.doubled(g, info))[0] == 0


def test_regression_list_is_chosen_by_the_model_alone(bases):
    """graph_match_cases.REGRESSION: per base graph, mutants that are safe by the model and whose run differs from the base run by at least
    100 x TOL in the final node or in a cache row the model writes, reads no float nothing wrote and writes no address twice - no matcher is
    asked here.  (That the matcher before this file accepted each
    of them is recorded in profiles/matcher_mutants.txt; that this one rejects them is the soundness test above.)"""
    total = 0
    for name, (g, info, inputs, base) in bases.items():
        muts = M.REGRESSION[name]
        corpus = set(GC.mutations(g))
        arr, _, _ = g.pack()
        for mut in muts:
            assert mut in corpus, (name, mut)
            with GC.Mutated(g, arr, mut):
                assert R.graph_fault(g) is None, (name, mut)
                trace = []
                identical, final, bufs = base.mutant(g, mut[0], trace)
                margin = M.margin(base, final, bufs)
            assert not identical and 100 * M.TOL <= margin < float("inf"), (name, M.describe(g, mut), margin)
            # a device can repeat the run: no node writes an address twice (the walk's "last write wins" has no parallel counterpart)
            assert all(np.unique(res.offs).size == res.offs.size for _, res in trace), (name, M.describe(g, mut))
        total += len(muts)
    assert 10 <= total <= 40
