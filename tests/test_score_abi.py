"""not-gpu: the scoring entry points (lh_score_rows, lh_llama_score; llamago_ScoreRows, llamago_Score, llamago_Perplexity) are declared and
exported, lh_row_score has the layout the ctypes / numpy views assume, and nothing of it works without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_NAMES = ("lh_score_rows", "lh_llama_score")
GO_NAMES = ("llamago_ScoreRows", "llamago_Score", "llamago_Perplexity")
FIELDS = (("logprob", 0), ("lse", 8), ("target_logit", 16), ("max_logit", 20), ("argmax", 24), ("target_rank", 28))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_score_entry_points_are_declared_and_exported(built):
    import llama_go_amd as pkg
    hip_hdr, ext_hdr = _header("llamahip.h"), _header("llamago_ext.h")
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    for n in HIP_NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hip_hdr), f"include/llamahip.h does not declare {n}"
        assert hasattr(hip, n), f"libllamahip.so does not export {n}"
    go = C.CDLL(pkg.LIBLLAMAGO)
    raw = open(os.path.join(ROOT, "include", "llamago_ext.h")).read()
    product_part = raw.split("[product] device plumbing", 1)[1]          # (names above the marker would have to exist in the checker too)
    assert all(re.search(r"\b" + n + r"\s*\(", ext_hdr) for n in GO_NAMES)
    for n in GO_NAMES:
        assert re.search(r"\b" + n + r"\s*\(", product_part), f"include/llamago_ext.h does not declare {n} in its [product] part"
        assert hasattr(go, n), f"libllamago.so does not export {n}"
    # the mirror of the reference's own names does not grow
    assert not re.search(r"Score|Perplexity", _header("llamago.h"))
    # the cgo shim has its wrapper over the C-ABI entry
    shim = open(os.path.join(ROOT, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    assert re.search(r"\bC\.lh_llama_score\s*\(", shim)


def test_row_score_layout_is_the_same_in_c_ctypes_and_numpy(built, tmp_path):
    from llama_go_amd.mlapi import ROW_SCORE_DTYPE, RowScore
    assert C.sizeof(RowScore) == 32
    assert ROW_SCORE_DTYPE.itemsize == 32
    for name, off in FIELDS:
        assert getattr(RowScore, name).offset == off, name
        assert ROW_SCORE_DTYPE.fields[name][1] == off, name
    assert [f[0] for f in RowScore._fields_] == [n for n, _ in FIELDS] == list(ROW_SCORE_DTYPE.names)
    # what a C compiler makes of the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "llamahip.h"\nint main(void) {\n  printf("%zu", sizeof(lh_row_score));\n'
                   + "".join(f'  printf(" %zu", offsetof(lh_row_score, {n}));\n' for n, _ in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32] + [off for _, off in FIELDS]


def test_scoring_fails_loudly_without_a_context_or_a_gpu(built):
    """No CPU path exists: a NULL handle is LH_EINVAL at the C-ABI, an error at the host library; without a HIP device the op-level entry cannot
    even get its context."""
    import numpy as np
    import llama_go_amd as pkg
    from llama_go_amd.mlapi import MLError, RowScore, load_product, score_rows
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    out = (RowScore * 1)()
    lg = (C.c_float * 8)()
    tg = (C.c_uint32 * 1)(0)
    hip.lh_score_rows.restype = hip.lh_llama_score.restype = C.c_int
    hip.lh_score_rows.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(RowScore)]
    hip.lh_llama_score.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(RowScore)]
    assert hip.lh_score_rows(None, lg, 1, 8, tg, out) == -1      # LH_EINVAL
    assert hip.lh_llama_score(None, tg, 1, 0, None, out) == -1
    prod = load_product()
    prod.lib.llamago_Score.restype = prod.lib.llamago_Perplexity.restype = C.c_int
    prod.lib.llamago_Score.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(RowScore)]
    prod.lib.llamago_Perplexity.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    assert prod.lib.llamago_Score(None, None, tg, 1, 0, None, out) != 0
    assert b"llamago_Score" in prod.lib.ml_LastError()
    nll, cnt = C.c_double(0), C.c_uint64(0)
    assert prod.lib.llamago_Perplexity(None, None, tg, 1, 0, C.byref(nll), C.byref(cnt)) != 0
    hip.lh_device_count.restype = C.c_int
    if hip.lh_device_count() == 0:
        with pytest.raises(MLError, match="no HIP"):
            score_rows(prod, np.zeros((1, 8), np.float32), [0])
