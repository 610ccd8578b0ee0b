"""not-gpu: lh_graph_match (csrc/graph_match.h, weight()) on Eval graphs whose weight matrices are f16 (dtype 1 = ml.TYPE_F16).  The graphs are the
mirror's own Eval graphs (tests/test_graph_check_cpu.py eval_graph) with the dtype of tensors and buffer extents rewritten; the matcher is built the
way tests/test_graph_match_cpu.py builds it.  Matrices may be f32, f16 or block-int8, all of one dtype within a model; norm vectors and the embedding
table stay f32; a tensor whose dtype differs from its buffer's stays refused."""
import ctypes as C

import pytest

import graph_match_cases as M
import graph_ops_ref as R
import test_graph_check_cpu as GC
from llama_go_amd.mlapi import SHAPES

CTX = 64
CASES = ((3, 0), (1, 5))   # (N, past): a prompt and a one-token step (the graph llama.Eval builds once per generated token)


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


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"N{c[0]}_past{c[1]}")
def base(request, mirror, match):
    N, past = request.param
    g = GC.eval_graph(mirror, "tiny", N, past, ctx=CTX)
    rc, info = match(g)
    assert rc == 1 and info["wtype"] == 0
    assert info == M.info_as_built(g, SHAPES["tiny"], N, past, CTX)
    return g, info


def matrix_leafs(info):
    """leaf indices of the 7 * L + 1 weight matrices of an lh_match_info (weights: 9 per layer - attention_norm, wq, wk, wv, wo, ffn_norm, w1, w2, w3 -
    then tok_embeddings, norm, output)"""
    L, w = info["L"], info["weights"]
    mats = [w[9 * il + k] for il in range(L) for k in (1, 2, 3, 4, 6, 7, 8)]
    return mats + [w[9 * L + 2]]


def set_dtype(g, leaf, dtype, tensor=True, buffer=True):
    t = g.t[leaf]
    if tensor:
        t.dtype = dtype
    if buffer:
        g.bufs[t.buf] = (g.bufs[t.buf][0], dtype)


def as_f16(g, info):
    h = g.copy()
    for leaf in matrix_leafs(info):
        set_dtype(h, leaf, 1)
    return h


def test_f16_matrices_match_with_wtype_1(base, match):
    g, info = base
    rc, got = match(as_f16(g, info))
    assert rc == 1
    assert got["wtype"] == 1
    assert {k: v for k, v in got.items() if k != "wtype"} == {k: v for k, v in info.items() if k != "wtype"}


def test_one_f32_matrix_among_f16_ones_is_refused(base, match):
    g, info = base
    mats = matrix_leafs(info)
    for leaf in (mats[0], mats[3], mats[len(mats) // 2], mats[-1]):   # the first wq, a wo, a matrix of a later layer, output
        h = as_f16(g, info)
        set_dtype(h, leaf, 0)
        assert match(h)[0] == 0, leaf
    h = g.copy()   # and the other way round: one f16 matrix in an f32 model
    set_dtype(h, mats[1], 1)
    assert match(h)[0] == 0


def test_f16_norm_vector_or_embedding_table_is_refused(base, match):
    g, info = base
    L, w = info["L"], info["weights"]
    for leaf in (w[0], w[5], w[9 * L + 1], w[9 * L + 0]):   # attention_norm, ffn_norm of layer 0, the final norm, tok_embeddings
        for start in (g, as_f16(g, info)):
            h = start.copy()
            set_dtype(h, leaf, 1)
            assert match(h)[0] == 0, leaf


def test_tensor_dtype_that_differs_from_its_buffer_is_refused(base, match):
    g, info = base
    mats = matrix_leafs(info)
    h = g.copy()   # tensors say f16, every buffer is f32
    for leaf in mats:
        set_dtype(h, leaf, 1, buffer=False)
    assert match(h)[0] == 0
    h = g.copy()   # one f16 tensor over an f32 buffer
    set_dtype(h, mats[0], 1, buffer=False)
    assert match(h)[0] == 0
    h = as_f16(g, info)   # an f32 tensor over an f16 buffer
    set_dtype(h, mats[-1], 0, buffer=False)
    assert match(h)[0] == 0


def test_node_path_names_f16_when_it_refuses_the_matrix(base, hip):
    """lh_graph_check on the f16 graph: a MulMat over a dtype-1 weight is refused like a block-int8 one, with a message that names f16"""
    g, info = base
    M.bind(hip)
    arr, ext, nb = as_f16(g, info).pack()
    msg = C.create_string_buffer(512)
    rc = hip.lh_graph_check(arr, g.n_leafs, g.total - g.n_leafs, ext, nb, msg, len(msg))
    assert rc == -4 and b"f16" in msg.value, (rc, msg.value)   # LH_EUNSUPPORTED
