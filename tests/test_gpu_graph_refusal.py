"""-m gpu: graphs the node path cannot serve safely are refused on the host, before anything is enqueued, and leave the context usable.

Each representative of tests/node_op_cases.refused_cases (one per hole the node path used to have: negative or missing sources, destinations
smaller than what the kernel writes, stride rules that leave the owner, empty or odd extents, parameters that cannot be cast) is FIRST passed to
lh_graph_check inside the test, which fails there - without calling lh_graph_compute - if the check accepts it: no graph that could reach a
kernel out of range is ever sent to a GPU.  That the check refuses every unsafe graph is proven on the CPU (tests/test_graph_check_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import node_op_cases as cases
import node_path_abi as abi

pytestmark = pytest.mark.gpu

REFUSED = cases.refused_cases()


@pytest.fixture(scope="module")
def session(product):
    import llama_go_amd as pkg
    s = abi.Session(abi.bind(C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)))
    yield s
    s.close()


@pytest.mark.parametrize("flags", [abi.NO_FUSION, 0], ids=["no_fusion", "fusion_allowed"])
@pytest.mark.parametrize("name,g,bad,words", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_on_the_host_before_any_launch(session, name, g, bad, words, flags):
    want, msg = session.check(g)
    assert want < 0, f"lh_graph_check accepts {name}: not sent to the GPU"
    assert words in msg, msg
    rc, trace = abi.trace_of(session.lib, lambda: session.compute(g, flags))
    assert rc == want, (rc, want, session.error())
    assert words in session.error(), session.error()
    assert trace == [], f"launched before the graph was refused: {trace}"      # (the graph's first node is a well-formed g_mul_mat)
    rc, _ = session.node_read(g.n_leafs, 1)
    assert rc < 0, "lh_node_read serves a node of a refused graph"
    # the same context then computes a well-formed graph
    good, z = cases.raw_abi_graph()
    assert session.check(good)[0] == 0
    assert session.compute(good, flags) == 0, session.error()
    rc, out = session.node_read(good.total - 1, z.size)
    assert rc == 0, session.error()
    assert np.abs(out.reshape(z.shape) - z).max() / z.max() < 1e-5
