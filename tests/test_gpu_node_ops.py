"""-m gpu: every generic kernel of the node path (csrc/kernels_generic.h, run_node of csrc/graph.hip) on strided views, through the raw C-ABI with
LH_GRAPH_NO_FUSION, against the reference model of op addressing and arithmetic (tests/graph_ops_ref.py): element by element within the
a-priori bound of the op (module docstring there; bit for bit for copies, masks and single fp32 operations), and - since sources and
destinations are windows inside larger registered buffers filled with a sentinel pattern - every float the model did not write must keep its
bits.  The cases are tests/node_op_cases.py; each is first accepted by lh_graph_check on the host."""
import numpy as np
import pytest

import graph_ops_ref as R
import node_op_cases as cases
import node_path_abi as abi

pytestmark = pytest.mark.gpu

CASES = cases.accepted_cases()


@pytest.fixture(scope="module")
def session(product):
    import ctypes as C
    import llama_go_amd as pkg
    s = abi.Session(abi.bind(C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)))
    yield s
    s.close()


def run_and_compare(session, case, want_trace=None):
    model = R.run(case.g, case.inputs)
    g, handle = session.bound_graph(case.g, case.inputs)
    try:
        rc, msg = session.check(g)
        assert rc == 0, f"lh_graph_check refuses {case.name}: {msg}"
        rc, trace = abi.trace_of(session.lib, lambda: session.compute(g, abi.NO_FUSION))
        assert rc == 0, session.error()
        if want_trace is not None:
            assert trace == want_trace, trace
        assert model.nodes, "the case computes nothing"
        got = {}
        for i, t in enumerate(case.g.t):
            if t.storage == i and t.buf:
                got[i] = session.read_buf(handle[t.buf], model.mem[i].size)
        problems = R.judge(case.g, case.inputs, model, got)
        assert not problems, f"{case.name}: " + "; ".join(problems)
        return model, got
    finally:
        session.free_buffers()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_op_on_views_matches_the_model_and_leaves_the_rest_alone(session, case):
    want = ["g_mul_mat"] if case.name.startswith("mul_mat") else []
    model, got = run_and_compare(session, case, want_trace=want)
    if case.name.startswith("rope_mode1") and case.name.endswith(("past7", "past2047")):
        assert all(r.offs.size == 0 for r in model.nodes.values())          # mode 1 with past >= ne2 writes nothing: covered by the sentinel check
    if case.name.startswith("rope"):
        # partial rotation: the upper half of every row (dims = 64 of 128) is unchanged bit for bit - it is not in the model's written set
        assert all(((r.offs - cases.PAD) % 130 < 64).all() for r in model.nodes.values())


ROPE_LAYOUTS = {
    # name: Permute axes for a leaf of numpy shape (2, n2 positions, 128)
    "permuted_3d": (0, 2, 1, 3),      # ne = (128, 2 heads, n2): ns1 > ns2
    "4d_ne3_2": (0, 2, 3, 1),         # ne = (128, 1, n2, 2)
}


def rope_checker_graph(ml, ctx, x, axes, past, mode):
    """Rope of dims = 64 of 128 in place on a permuted view of the leaf x.  The result is a ViewTensor of that view (ml.go:1016): the leaf's data
    under packed strides, so the Cpy behind it (the API reads contiguous tensors) hands the leaf's array back in its own order."""
    from test_gpu_ops import leaf
    view = ml.Permute(ctx, leaf(ml, ctx, x), *axes)
    return ml.Copy(ctx, ml.Rope(ctx, view, past, 64, mode), ml.NewTensor(ctx, (128, x.shape[1], 2)))


@pytest.mark.parametrize("mode,n2,past", [(0, 3, 0), (0, 3, 5), (0, 3, 2047), (1, 7, 5), (1, 7, 7)])
@pytest.mark.parametrize("layout", sorted(ROPE_LAYOUTS))
def test_rope_on_strided_views_bit_for_bit_against_the_checker(product, oracle, layout, mode, n2, past):
    """the checker rotates in f64 from its own libm's cos / sin (oracle.c fwd_rope), g_rope from the f64 table the host builds: one rounding on
    both sides, so partial rotation on permuted 3-D and 4-D views agrees bit for bit, as the contiguous shapes of tests/test_gpu_ops.py do.
    The rotation is addressed by the SOURCE's strides (ml.go:2274-2281), not by the packed ones of the result."""
    from test_gpu_ops import Pair
    axes = ROPE_LAYOUTS[layout]
    x = cases.rng(13, mode, past).standard_normal((2, n2, 128)).astype(np.float32)
    out = Pair(product, oracle).run(lambda ml, ctx: rope_checker_graph(ml, ctx, x, axes, past, mode))
    hip, orc = (out[k][0].reshape(x.shape) for k in ("hip", "orc"))
    assert np.array_equal(hip.view(np.uint32), orc.view(np.uint32)), f"{np.count_nonzero(hip != orc)} elements differ"
    assert np.array_equal(hip[..., 64:].view(np.uint32), x[..., 64:].view(np.uint32))                    # the upper half is not rotated
    first = past if mode == 1 else 0
    assert np.array_equal(hip[:, :first].view(np.uint32), x[:, :first].view(np.uint32))                  # mode 1: positions below past keep their bits
    if first < n2:
        assert not np.array_equal(hip[:, first:, :64], x[:, first:, :64])                                # and the rest did turn (position 0 is the identity)


def test_cpy_grid_stride_second_lap(session):
    """ne = (4100, 4100): more elements than 65535 blocks x 256 threads, so the grid-stride loop of every generic kernel's launch shape runs again"""
    assert 4100 * 4100 > 65535 * 256
    run_and_compare(session, cases.big_cpy_case())
