"""not-gpu: lh_graph_match (csrc/graph_match.h, weight()) on Eval graphs whose weight matrices are block-int4 (dtype 2 = ml.TYPE_Q4_0), built like
tests/test_f16_match_cpu.py: the mirror's own Eval graphs with the dtype of tensors and buffer extents rewritten.  Matrices may be f32, f16, block-int4 or
block-int8, all of one dtype within a model, block-int4 under block-int8's shape rule (the buffer holds exactly ne0 * ne1 logical elements); norm vectors
and the embedding table stay f32; a tensor whose dtype differs from its buffer's stays refused."""
import ctypes as C

import pytest

import graph_match_cases as M
import test_f16_match_cpu as F
from test_f16_match_cpu import hip, mirror, match, base, matrix_leafs, set_dtype   # noqa: F401  (fixtures)


def as_q4(g, info):
    h = g.copy()
    for leaf in matrix_leafs(info):
        set_dtype(h, leaf, 2)
    return h


def test_q4_matrices_match_with_wtype_2(base, match):
    g, info = base
    rc, got = match(as_q4(g, info))
    assert rc == 1
    assert got["wtype"] == 2
    assert {k: v for k, v in got.items() if k != "wtype"} == {k: v for k, v in info.items() if k != "wtype"}


def test_mixed_dtypes_are_refused(base, match):
    g, info = base
    mats = matrix_leafs(info)
    for other in (0, 1, 7):
        for leaf in (mats[0], mats[3], mats[len(mats) // 2], mats[-1]):
            h = as_q4(g, info)
            set_dtype(h, leaf, other)
            assert match(h)[0] == 0, (leaf, other)
    for start in (g, F.as_f16(g, info)):   # and the other way round: one block-int4 matrix in an f32 / f16 model
        h = start.copy()
        set_dtype(h, mats[1], 2)
        assert match(h)[0] == 0


def test_q4_norm_vector_or_embedding_table_is_refused(base, match):
    g, info = base
    L, w = info["L"], info["weights"]
    for leaf in (w[0], w[5], w[9 * L + 1], w[9 * L + 0]):   # attention_norm, ffn_norm of layer 0, the final norm, tok_embeddings
        for start in (g, as_q4(g, info)):
            h = start.copy()
            set_dtype(h, leaf, 2)
            assert match(h)[0] == 0, leaf


def test_tensor_dtype_that_differs_from_its_buffer_is_refused(base, match):
    g, info = base
    mats = matrix_leafs(info)
    h = g.copy()   # tensors say block-int4, every buffer is f32
    for leaf in mats:
        set_dtype(h, leaf, 2, buffer=False)
    assert match(h)[0] == 0
    h = as_q4(g, info)   # an f32 tensor over a block-int4 buffer
    set_dtype(h, mats[-1], 0, buffer=False)
    assert match(h)[0] == 0
    h = as_q4(g, info)   # a block-int8 tensor over a block-int4 buffer
    set_dtype(h, mats[0], 7, buffer=False)
    assert match(h)[0] == 0


def test_q4_matrix_whose_extent_is_not_its_shape_is_refused(base, match):
    g, info = base
    mats = matrix_leafs(info)
    for leaf in (mats[0], mats[-1]):
        for delta in (32, -32):
            h = as_q4(g, info)
            buf = h.t[leaf].buf
            h.bufs[buf] = (h.bufs[buf][0] + delta, 2)
            assert match(h)[0] == 0, (leaf, delta)
        h = g.copy()   # (an f32 matrix may sit in a larger buffer: the rule is the block formats')
        buf = h.t[leaf].buf
        h.bufs[buf] = (h.bufs[buf][0] + 32, 0)
        assert match(h)[0] == 1


def test_node_path_names_int4_when_it_refuses_the_matrix(base, hip):
    """lh_graph_check on the block-int4 graph: a MulMat over a dtype-2 weight is refused like the others, with a message that names block-int4"""
    g, info = base
    M.bind(hip)
    arr, ext, nb = as_q4(g, info).pack()
    msg = C.create_string_buffer(512)
    rc = hip.lh_graph_check(arr, g.n_leafs, g.total - g.n_leafs, ext, nb, msg, len(msg))
    assert rc == -4 and b"int4" in msg.value, (rc, msg.value)   # LH_EUNSUPPORTED
