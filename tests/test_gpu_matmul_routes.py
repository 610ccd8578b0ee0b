"""Every kernel instantiation a node-path MulMat can take (lh_graph_compute -> gemm_small_n, csrc/plan.hip; g_mul_mat, csrc/graph.hip), each
held element by element to a float64 product and to the checker's own accuracy, with non-finite and extreme operands.

Each case of ROUTES names the instantiation its shape must take; the per-thread route trace (include/llamahip.h lh_route_trace) has to show
exactly that list of launches.  A re-tuned cost constant that moves a case to another kernel fails here instead of silently testing
something else.

The bound, one constant for every route:
    |y - y64|_i  <=  C * 2^-24 * sum_k |x_ik w_mk|
C = 16.  cdna_hip_programming.md (FP32-input MFMA) quotes 0.75-3.5e-7 * sum|ab| (1.3-5.9 units of 2^-24) up to K = 4096 for the fp32 matrix
pipe; the cases here reach K = 24576 on the register-tile kernel, whose per-thread sequential depth grows with K, and the result carries one
more rounding of its own.  Not measured on the hardware to be tight: test_bound_is_sharp shows that what a subtly wrong kernel produces
breaks it by orders of magnitude.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from llama_go_amd.mlapi import route_trace

BOUND_C = 16.0
U = 2.0 ** -24


# ---- the bound and its sharpness (no GPU) ----------------------------------------------------------------------------------------------

def exact_product(x, w):
    """f64 product and the per-element scale sum_k |x_ik w_mk| of x [..., n, K] and w [..., M, K]."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    return x64 @ np.swapaxes(w64, -1, -2), np.abs(x64) @ np.swapaxes(np.abs(w64), -1, -2)


def bound_violations(y, y64, scale):
    """Number of elements outside the bound (NaN counts as outside)."""
    err = np.abs(y.astype(np.float64) - y64)
    return int(np.count_nonzero(~(err <= BOUND_C * U * scale)))


def split3_np(a):
    """numpy restatement of split3 (csrc/kernels_common.h) for finite fp32 a: hi + mid + lo == a exactly."""
    a = np.asarray(a, np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = (a - hi).astype(np.float32)
    mid = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    lo = (r1 - mid).astype(np.float32)
    return hi, mid, lo


def test_bound_is_sharp():
    """The element-wise bound fails what a subtly wrong kernel would return: a dropped xm * wh product, one 32-wide K slab dropped or counted
    twice, one output element taken from the neighbouring row of its tile.  (And holds for the fp32 sum itself.)"""
    r = np.random.default_rng(7)
    n, M, K = 24, 64, 512
    x = r.standard_normal((n, K), dtype=np.float32)
    w = (r.standard_normal((M, K), dtype=np.float32) / np.float32(np.sqrt(K))).astype(np.float32)
    y64, scale = exact_product(x, w)
    y32 = (x @ w.T).astype(np.float32)                              # an fp32 blocked sum: inside
    assert bound_violations(y32, y64, scale) == 0
    xh, xm, _ = split3_np(x)
    wh, _, _ = split3_np(w)
    mutants = {
        "dropped xm*wh": y64 - xm.astype(np.float64) @ wh.astype(np.float64).T,
        "slab 3 dropped": y64 - x[:, 96:128].astype(np.float64) @ w[:, 96:128].astype(np.float64).T,
        "slab 5 twice": y64 + x[:, 160:192].astype(np.float64) @ w[:, 160:192].astype(np.float64).T,
    }
    nb = y64.copy()
    nb[5, 17] = y64[6, 17]                                          # row 5 of a 16-row tile reads row 6's sum
    mutants["neighbour row"] = nb
    for name, y in mutants.items():
        assert bound_violations(y.astype(np.float32), y64, scale) > 0, f"the bound does not see: {name}"


def ieee_reference(x, w):
    """Order-independent IEEE outcome of sum_k x_ik w_mk for operands with inf / NaN: NaN where a term is NaN (NaN operand, inf * 0) or where
    +inf and -inf terms meet, +-inf where the only non-finite terms are infinities of one sign, 0 where every term is finite.  Built from the
    non-finite operands only (x [n, K], w [M, K]; finite products do not overflow in f64)."""
    n, M = x.shape[0], w.shape[0]
    nan, pos, neg = (np.zeros((n, M), bool) for _ in range(3))
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    with np.errstate(invalid="ignore"):
        for i, k in np.argwhere(~np.isfinite(x)):
            t = x64[i, k] * w64[:, k]
            nan[i] |= np.isnan(t); pos[i] |= t == np.inf; neg[i] |= t == -np.inf
        for m, k in np.argwhere(~np.isfinite(w)):
            t = x64[:, k] * w64[m, k]
            nan[:, m] |= np.isnan(t); pos[:, m] |= t == np.inf; neg[:, m] |= t == -np.inf
    out = np.zeros((n, M))
    out[pos] = np.inf
    out[neg] = -np.inf
    out[nan | (pos & neg)] = np.nan
    return out


def test_ieee_reference_helper():
    """(no GPU) the special-value model itself: inf * 0 and inf - inf are NaN, one-signed infinities survive, NaN payloads stay NaN."""
    x = np.array([[1.0, 0.0], [1.0, 1.0], [np.nan, 1.0], [1.0, -1.0]], np.float32)
    w = np.array([[np.inf, 1.0], [np.inf, np.inf], [1.0, 2.0]], np.float32)
    ref = ieee_reference(x, w)
    assert ref[0, 0] == np.inf and np.isnan(ref[0, 1]) and ref[0, 2] == 0
    assert np.isnan(ref[2]).all()
    assert ref[3, 0] == np.inf and np.isnan(ref[3, 1])


# ---- the route table -------------------------------------------------------------------------------------------------------------------

def cols(ki, u, nc, passes=1):
    return [f"k_gemv_cols<{ki},{u},1024,{nc}>"] * passes


# id: (M, K, n, expected trace of clean operands, expected trace when the operands hold values outside the bf16 split's exact range, or
#      None when it is the same).  MI355X, 256 CUs.
ROUTES = {
    # k_gemv_cols: one token row, or K not a multiple of 128 / 32; ki = ceil(K / 4096) picks the instantiation, NC columns per pass
    "cols_ki1": (300, 4096, 1, cols(1, 2, 8), None),
    "cols_ki2_k4100": (257, 4100, 1, cols(2, 2, 8), None),
    "cols_ki2_ragged": (256, 4100, 9, cols(2, 2, 8, 2), None),          # 8 + 1 columns
    "cols_ki3": (256, 8196, 3, cols(3, 2, 4), None),
    "cols_ki4_ragged": (300, 12292, 5, cols(4, 1, 4, 2), None),         # 4 + 1
    "cols_ki5_ragged": (256, 16388, 3, cols(5, 1, 2, 2), None),         # 2 + 1
    "cols_ki6": (260, 24576, 1, cols(6, 1, 2), None),
    # k_stream_mm2 (2..16 rows, one column tile): MAXT = ceil(M / 16 / 256) row tiles per workgroup
    "mm2_t1_n2": (4096, 4096, 2, ["k_stream_mm2<1,1,128>/s1"], None),
    "mm2_t1_kc256_n8": (4096, 8192, 8, ["k_stream_mm2<1,1,256>/s1"], None),
    "mm2_t2_n9": (8192, 512, 9, ["k_stream_mm2<2,1,128>/s1"], None),
    "mm2_t3_n16": (12288, 512, 16, ["k_stream_mm2<3,1,128>/s1"], None),
    "mm2_t4_n5": (16384, 256, 5, ["k_stream_mm2<4,1,128>/s1"], None),
    "mm2_t6_n3": (20480, 256, 3, ["k_stream_mm2<6,1,128>/s1"], None),
    # k_stream_dma (17..128 rows): NCT = ceil(n / 16) column tiles
    "dma_t1_n17": (4096, 1024, 17, ["k_stream_dma<1,2,64,4,0,1>/s1"], None),
    "dma_t2_n33": (8192, 512, 33, ["k_stream_dma<2,3,64,4,0,1>/s1"], None),
    "dma_t1_n64": (256, 1024, 64, ["k_stream_dma<1,4,64,4,0,1>/s1"], None),
    "dma_t1_n65": (256, 1024, 65, ["k_stream_dma<1,5,64,4,0,1>/s1"], None),
    "dma_t1_n128": (4096, 512, 128, ["k_stream_dma<1,8,64,4,0,2>/s1"], None),
    "dma_t6_n24": (20480, 256, 24, ["k_stream_dma<6,2,128,2,0,1>/s1"], None),
    # tile GEMMs: M not a multiple of 16 keeps the stream kernels out.  Up to 64 rows: 64 x 128 tiles; K < 16 GBK = 512 register-staged
    "mfma_k480": (260, 480, 20, ["k_gemm_mfma<2,2,1,2>"], None),
    "glds_k512": (260, 512, 20, ["k_gemm_glds<2,2,1,2>/s1", ], None),
    "glds_n64_split": (260, 4096, 64, ["k_gemm_glds<2,2,1,2>/s8", "k_splitk_reduce"], None),
    "glds_2221_n65": (260, 512, 65, ["k_gemm_glds<2,2,2,1>/s1"], None),
    "glds_2221_split": (260, 2048, 65, ["k_gemm_glds<2,2,2,1>/s4", "k_splitk_reduce"], None),
    "glds_2221_ragged_m": (301, 1024, 129, ["k_gemm_glds<2,2,2,1>/s1"], None),   # M % 4 != 0: no split-K
    "glds_2222": (8196, 512, 129, ["k_gemm_glds<2,2,2,2>/s1"], None),
    "glds_4115_split": (4100, 4096, 65, ["k_gemm_glds<4,1,1,5>/s8", "k_splitk_reduce"], None),
    # k_gemm_b9 (bf16 exact split, > 128 rows), split-K off and on; with operands outside the split's exact range the fp32 GEMM
    "b9_s1": (4100, 512, 1000, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s1"], ["k_gemm_glds<4,1,1,5>/s1"]),
    "b9_s4": (4100, 2048, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s4", "k_splitk_reduce"], ["k_gemm_glds<4,1,1,5>/s4", "k_splitk_reduce"]),
    "b9_s8": (2052, 4096, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s8", "k_splitk_reduce"], ["k_gemm_glds<4,1,1,5>/s8", "k_splitk_reduce"]),
    "b9_s2": (8196, 1024, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s2", "k_splitk_reduce"], ["k_gemm_glds<4,1,1,5>/s2", "k_splitk_reduce"]),
    "b9_s3": (8196, 2048, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s3", "k_splitk_reduce"], ["k_gemm_glds<4,1,1,5>/s2", "k_splitk_reduce"]),
    "b9_s5": (6148, 8192, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s5", "k_splitk_reduce"], ["k_gemm_glds<2,2,2,2>/s2", "k_splitk_reduce"]),
    "b9_s6": (5124, 4096, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s6", "k_splitk_reduce"], ["k_gemm_glds<2,2,2,1>/s1"]),
    "b9_s7": (4100, 4096, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s7", "k_splitk_reduce"], ["k_gemm_glds<4,1,1,5>/s4", "k_splitk_reduce"]),
    "b9_s8_k8192": (3076, 8192, 129, ["k_split3_rows", "k_gemm_b9<1,8,4,1,2>/s8", "k_splitk_reduce"], ["k_gemm_glds<2,2,2,2>/s4", "k_splitk_reduce"]),
    # the other tile shapes and split-K factors the cost model picks (register-staged kernel: K < 512)
    "mfma_2221": (260, 32, 65, ["k_gemm_mfma<2,2,2,1>"], None),
    "mfma_2222": (8196, 32, 129, ["k_gemm_mfma<2,2,2,2>"], None),
    "mfma_4115": (4100, 32, 1000, ["k_gemm_mfma<4,1,1,5>"], None),
    "glds_2212_s2": (260, 1024, 9, ["k_gemm_glds<2,2,1,2>/s2", "k_splitk_reduce"], None),
    "glds_2212_s4": (260, 2048, 9, ["k_gemm_glds<2,2,1,2>/s4", "k_splitk_reduce"], None),
    "glds_2212_s16": (260, 8192, 9, ["k_gemm_glds<2,2,1,2>/s16", "k_splitk_reduce"], None),
    "glds_2212_s32": (260, 16384, 9, ["k_gemm_glds<2,2,1,2>/s32", "k_splitk_reduce"], None),
    "glds_2221_s2": (260, 1024, 65, ["k_gemm_glds<2,2,2,1>/s2", "k_splitk_reduce"], None),
    "glds_2221_s8": (260, 4096, 65, ["k_gemm_glds<2,2,2,1>/s8", "k_splitk_reduce"], None),
    "glds_2221_s16": (260, 8192, 65, ["k_gemm_glds<2,2,2,1>/s16", "k_splitk_reduce"], None),
    "glds_2221_s32": (260, 16384, 65, ["k_gemm_glds<2,2,2,1>/s32", "k_splitk_reduce"], None),
    "glds_2222_s8": (1540, 16384, 129, ["k_gemm_glds<2,2,2,2>/s8", "k_splitk_reduce"], None),
    "glds_4115_s2": (16388, 1024, 65, ["k_gemm_glds<4,1,1,5>/s2", "k_splitk_reduce"], None),
    "glds_4115_s16": (2052, 8192, 65, ["k_gemm_glds<4,1,1,5>/s16", "k_splitk_reduce"], None),
    "glds_4115_s32": (516, 16384, 129, ["k_gemm_glds<4,1,1,5>/s32", "k_splitk_reduce"], None),
    # g_mul_mat: narrow (M < 256) and K beyond 24576
    "gmm_narrow": (255, 1024, 7, ["g_mul_mat"], None),
    "gmm_k24580": (256, 24580, 2, ["g_mul_mat"], None),
    # the stream kernels over their grid: MAXT row tiles per workgroup (1, 2, 3, 4; 5 -> 6; 7 -> 8) x NCT = ceil(n / 16) column tiles, K = 256
    "stream_t1_n9": (4096, 256, 9, ["k_stream_mm2<1,1,128>/s1"], None),
    "stream_t1_n32": (4096, 256, 32, ["k_stream_dma<1,2,64,4,0,1>/s1"], None),
    "stream_t1_n47": (4096, 256, 47, ["k_stream_dma<1,3,64,4,0,1>/s1"], None),
    "stream_t1_n64": (4096, 256, 64, ["k_stream_dma<1,4,64,4,0,1>/s1"], None),
    "stream_t1_n79": (4096, 256, 79, ["k_stream_dma<1,5,64,4,0,1>/s1"], None),
    "stream_t1_n96": (4096, 256, 96, ["k_stream_dma<1,6,64,4,0,1>/s1"], None),
    "stream_t1_n111": (4096, 256, 111, ["k_stream_dma<1,7,64,4,0,1>/s1"], None),
    "stream_t1_n128": (4096, 256, 128, ["k_stream_dma<1,8,64,4,0,2>/s1"], None),
    "stream_t2_n9": (8192, 256, 9, ["k_stream_mm2<2,1,128>/s1"], None),
    "stream_t2_n32": (8192, 256, 32, ["k_stream_dma<2,2,64,4,0,1>/s1"], None),
    "stream_t2_n47": (8192, 256, 47, ["k_stream_dma<2,3,64,4,0,1>/s1"], None),
    "stream_t2_n64": (8192, 256, 64, ["k_stream_dma<2,4,64,4,0,1>/s1"], None),
    "stream_t2_n79": (8192, 256, 79, ["k_stream_dma<2,5,64,4,0,1>/s1"], None),
    "stream_t2_n96": (8192, 256, 96, ["k_stream_dma<2,6,64,4,0,1>/s1"], None),
    "stream_t2_n111": (8192, 256, 111, ["k_stream_dma<2,7,64,4,0,1>/s1"], None),
    "stream_t2_n128": (8192, 256, 128, ["k_stream_dma<2,8,64,4,0,2>/s1"], None),
    "stream_t3_n9": (12128, 256, 9, ["k_stream_mm2<3,1,128>/s1"], None),
    "stream_t3_n32": (12128, 256, 32, ["k_stream_dma<3,2,64,4,0,1>/s1"], None),
    "stream_t3_n47": (12128, 256, 47, ["k_stream_dma<3,3,64,4,0,1>/s1"], None),
    "stream_t3_n64": (12128, 256, 64, ["k_stream_dma<3,4,64,4,0,1>/s1"], None),
    "stream_t3_n79": (12128, 256, 79, ["k_stream_dma<3,5,64,4,0,1>/s1"], None),
    "stream_t3_n96": (12128, 256, 96, ["k_stream_dma<3,6,64,4,0,1>/s1"], None),
    "stream_t3_n111": (12128, 256, 111, ["k_stream_dma<3,7,64,4,0,1>/s1"], None),
    "stream_t3_n128": (12128, 256, 128, ["k_stream_dma<3,8,64,3,0,2>/s1"], None),
    "stream_t4_n9": (16384, 256, 9, ["k_stream_mm2<4,1,128>/s1"], None),
    "stream_t4_n32": (16384, 256, 32, ["k_stream_dma<4,2,64,4,0,1>/s1"], None),
    "stream_t4_n47": (16384, 256, 47, ["k_stream_dma<4,3,64,4,0,1>/s1"], None),
    "stream_t4_n64": (16384, 256, 64, ["k_stream_dma<4,4,64,4,0,1>/s1"], None),
    "stream_t4_n79": (16384, 256, 79, ["k_stream_dma<4,5,64,4,0,1>/s1"], None),
    "stream_t4_n96": (16384, 256, 96, ["k_stream_dma<4,6,64,4,0,1>/s1"], None),
    "stream_t4_n111": (16384, 256, 111, ["k_stream_dma<4,7,64,3,0,1>/s1"], None),
    "stream_t4_n128": (16384, 256, 128, ["k_stream_dma<4,8,64,3,0,2>/s1"], None),
    "stream_t6_n9": (20480, 256, 9, ["k_stream_mm2<6,1,128>/s1"], None),
    "stream_t6_n32": (20480, 256, 32, ["k_stream_dma<6,2,128,2,0,1>/s1"], None),
    "stream_t6_n47": (20480, 256, 47, ["k_stream_dma<6,3,64,4,0,1>/s1"], None),
    "stream_t6_n64": (20480, 256, 64, ["k_stream_dma<6,4,64,4,0,1>/s1"], None),
    "stream_t6_n79": (20480, 256, 79, ["k_stream_dma<6,5,64,3,0,1>/s1"], None),
    "stream_t6_n96": (20480, 256, 96, ["k_stream_dma<6,6,64,3,0,1>/s1"], None),
    "stream_t6_n111": (20480, 256, 111, ["k_stream_dma<6,7,64,3,0,1>/s1"], None),
    "stream_t6_n128": (20480, 256, 128, ["k_stream_dma<6,8,64,2,0,2>/s1"], None),
    "stream_t8_n9": (28688, 256, 9, ["k_stream_mm2<8,1,128>/s1"], None),
    "stream_t8_n32": (28688, 256, 32, ["k_stream_dma<8,2,128,2,0,1>/s1"], None),
    "stream_t8_n47": (28688, 256, 47, ["k_stream_dma<8,3,64,3,0,1>/s1"], None),
    "stream_t8_n64": (28688, 256, 64, ["k_stream_dma<8,4,64,3,0,1>/s1"], None),
}
# batched 3-D operands and a strided (permuted) weight: g_mul_mat
BATCHED = {
    "gmm_batched3d": (96, 256, 5, 3, False, ["g_mul_mat"]),
    "gmm_strided_w": (64, 128, 9, 2, True, ["g_mul_mat"]),
}

# Every instantiation the node path can launch (gemm_small_n -> gemm_stream_group / gemm_mfma_group, plan.hip; g_mul_mat, graph.hip), written
# out from the dispatch, not from the table above:
#   k_gemv_cols<KI, U, 1024, NC>, KI = ceil(K / 4096) = 1..6;
#   k_stream_mm2<MAXT, 1, KC> (one column tile, 2..16 rows; KC = 256 only for MAXT = 1, K > 4096, K % 256 == 0), MAXT in 1, 2, 3, 4, 6, 8;
#   k_stream_dma<MAXT, NCT, KC, NIMG, 0, CS> for NCT = 2..8 (MAXT = 8: up to 4) - NIMG = min(4, 40 / (MAXT + NCT)), 128-column chunks in two
#     images for NCT = 2 and MAXT >= 5, CS = 2 for NCT = 8;
#   k_gemm_mfma (K < 512) and k_gemm_glds in the four tile shapes, the latter with split-K 1..32 (pick_splitk) and its reduce pass;
#   k_gemm_b9 with split-K 1..8 behind k_split3_rows.
NODE_PATH_INSTANTIATIONS = {
    "k_gemv_cols<1,2,1024,8>", "k_gemv_cols<2,2,1024,8>", "k_gemv_cols<3,2,1024,4>", "k_gemv_cols<4,1,1024,4>", "k_gemv_cols<5,1,1024,2>",
    "k_gemv_cols<6,1,1024,2>", "k_stream_mm2<1,1,128>/s1", "k_stream_mm2<1,1,256>/s1", "k_stream_mm2<2,1,128>/s1", "k_stream_mm2<3,1,128>/s1",
    "k_stream_mm2<4,1,128>/s1", "k_stream_mm2<6,1,128>/s1", "k_stream_mm2<8,1,128>/s1", "k_stream_dma<1,2,64,4,0,1>/s1",
    "k_stream_dma<1,3,64,4,0,1>/s1", "k_stream_dma<1,4,64,4,0,1>/s1", "k_stream_dma<1,5,64,4,0,1>/s1", "k_stream_dma<1,6,64,4,0,1>/s1",
    "k_stream_dma<1,7,64,4,0,1>/s1", "k_stream_dma<1,8,64,4,0,2>/s1", "k_stream_dma<2,2,64,4,0,1>/s1", "k_stream_dma<2,3,64,4,0,1>/s1",
    "k_stream_dma<2,4,64,4,0,1>/s1", "k_stream_dma<2,5,64,4,0,1>/s1", "k_stream_dma<2,6,64,4,0,1>/s1", "k_stream_dma<2,7,64,4,0,1>/s1",
    "k_stream_dma<2,8,64,4,0,2>/s1", "k_stream_dma<3,2,64,4,0,1>/s1", "k_stream_dma<3,3,64,4,0,1>/s1", "k_stream_dma<3,4,64,4,0,1>/s1",
    "k_stream_dma<3,5,64,4,0,1>/s1", "k_stream_dma<3,6,64,4,0,1>/s1", "k_stream_dma<3,7,64,4,0,1>/s1", "k_stream_dma<3,8,64,3,0,2>/s1",
    "k_stream_dma<4,2,64,4,0,1>/s1", "k_stream_dma<4,3,64,4,0,1>/s1", "k_stream_dma<4,4,64,4,0,1>/s1", "k_stream_dma<4,5,64,4,0,1>/s1",
    "k_stream_dma<4,6,64,4,0,1>/s1", "k_stream_dma<4,7,64,3,0,1>/s1", "k_stream_dma<4,8,64,3,0,2>/s1", "k_stream_dma<6,2,128,2,0,1>/s1",
    "k_stream_dma<6,3,64,4,0,1>/s1", "k_stream_dma<6,4,64,4,0,1>/s1", "k_stream_dma<6,5,64,3,0,1>/s1", "k_stream_dma<6,6,64,3,0,1>/s1",
    "k_stream_dma<6,7,64,3,0,1>/s1", "k_stream_dma<6,8,64,2,0,2>/s1", "k_stream_dma<8,2,128,2,0,1>/s1", "k_stream_dma<8,3,64,3,0,1>/s1",
    "k_stream_dma<8,4,64,3,0,1>/s1", "k_gemm_mfma<2,2,1,2>", "k_gemm_mfma<4,1,1,5>", "k_gemm_mfma<2,2,2,1>", "k_gemm_mfma<2,2,2,2>",
    "k_gemm_glds<2,2,1,2>/s1", "k_gemm_glds<2,2,1,2>/s2", "k_gemm_glds<2,2,1,2>/s4", "k_gemm_glds<2,2,1,2>/s8", "k_gemm_glds<2,2,1,2>/s16",
    "k_gemm_glds<2,2,1,2>/s32", "k_gemm_glds<4,1,1,5>/s1", "k_gemm_glds<4,1,1,5>/s2", "k_gemm_glds<4,1,1,5>/s4", "k_gemm_glds<4,1,1,5>/s8",
    "k_gemm_glds<4,1,1,5>/s16", "k_gemm_glds<4,1,1,5>/s32", "k_gemm_glds<2,2,2,1>/s1", "k_gemm_glds<2,2,2,1>/s2", "k_gemm_glds<2,2,2,1>/s4",
    "k_gemm_glds<2,2,2,1>/s8", "k_gemm_glds<2,2,2,1>/s16", "k_gemm_glds<2,2,2,1>/s32", "k_gemm_glds<2,2,2,2>/s1", "k_gemm_glds<2,2,2,2>/s2",
    "k_gemm_glds<2,2,2,2>/s4", "k_gemm_glds<2,2,2,2>/s8", "k_gemm_glds<2,2,2,2>/s16", "k_gemm_glds<2,2,2,2>/s32", "k_gemm_b9<1,8,4,1,2>/s1",
    "k_gemm_b9<1,8,4,1,2>/s2", "k_gemm_b9<1,8,4,1,2>/s3", "k_gemm_b9<1,8,4,1,2>/s4", "k_gemm_b9<1,8,4,1,2>/s5", "k_gemm_b9<1,8,4,1,2>/s6",
    "k_gemm_b9<1,8,4,1,2>/s7", "k_gemm_b9<1,8,4,1,2>/s8", "k_split3_rows", "k_splitk_reduce", "g_mul_mat",
}

# instantiations of the list no case reaches, each with the reason
EXEMPT = {
    "k_gemm_glds<2,2,2,2>/s16": "128 x 128 tiles win the cost model only where there are enough tiles that splits beyond 8 do not pay: a search of the "
                                "cost model over M 260..16400, K 512..16384, n 65..256 finds no plain 2-D shape that takes it",
    "k_gemm_glds<2,2,2,2>/s32": "as /s16",
}


def _bind(ml):
    ml.lib.llamago_GraphComputeNoFusion.restype = C.c_int
    ml.lib.llamago_GraphComputeNoFusion.argtypes = [C.c_void_p, C.c_void_p]


def leaf(ml, ctx, arr):
    arr = np.asarray(arr, dtype=np.float32)
    return ml.NewTensor(ctx, tuple(reversed(arr.shape)), data=arr)


def run_mulmat(ml, w, x, ctx=None, gpu=True, strided=False):
    """MulMat(w, x) on one library through one graph; returns (y [.., n, M], trace).  ctx given: run on it and keep it."""
    own = ctx is None
    if own:
        ctx = ml.NewContext(4, False, False)
    g = ml.NewGraph()
    try:
        if w.ndim == 2:
            t = ml.MulMat(ctx, leaf(ml, ctx, w), leaf(ml, ctx, x))
        else:
            B, M, K = w.shape
            if strided:   # the weight as a permuted view: memory [M][B][K], element (k, m, b) at m B K + b K + k
                W = ml.Permute(ctx, ml.Reshape3D(ctx, leaf(ml, ctx, np.ascontiguousarray(w.transpose(1, 0, 2)).reshape(-1)), K, B, M), 0, 2, 1, 3)
            else:
                W = ml.Reshape3D(ctx, leaf(ml, ctx, w.reshape(-1)), K, M, B)
            t = ml.MulMat(ctx, W, ml.Reshape3D(ctx, leaf(ml, ctx, x.reshape(-1)), K, x.shape[1], B))
        ml.BuildForwardExpand(g, t)
        if gpu:
            _bind(ml)
            rc, trace = route_trace(lambda: ml.lib.llamago_GraphComputeNoFusion(ctx, g))
            if rc:
                raise RuntimeError(ml.last_error())
        else:
            ml.GraphCompute(ctx, g)
            trace = []
        y = ml.read(ctx, t).copy()
    finally:
        ml.FreeGraph(g)
        if own:
            ml.ReleaseContext(ctx)
    out_shape = x.shape[:-1] + (w.shape[-2],)
    return y.reshape(out_shape), trace


def operands(M, K, n, seed, B=None):
    r = np.random.default_rng(seed)
    lead = (B,) if B else ()
    x = r.standard_normal(lead + (n, K), dtype=np.float32)
    w = (r.standard_normal(lead + (M, K), dtype=np.float32) / np.float32(np.sqrt(K))).astype(np.float32)
    x.flat[:: 97] = 0.0
    x.flat[1:: 193] = -0.0                                              # signed zeros among the operands
    return x, w


def rel_errors(y, y64, scale):
    e = np.abs(y.astype(np.float64) - y64) / np.maximum(scale, np.finfo(np.float64).tiny)
    return float(np.sqrt(np.mean(e * e))), float(e.max())


def check_clean(y, y_orc, x, w, label):
    y64, scale = exact_product(x, w)
    bad = bound_violations(y, y64, scale)
    assert bad == 0, f"{label}: {bad} elements outside C 2^-24 sum|xw| (worst {np.nanmax(np.abs(y - y64) / scale):.3e} sum|xw|)"
    g_rms, g_max = rel_errors(y, y64, scale)
    o_rms, o_max = rel_errors(y_orc, y64, scale)
    assert g_rms <= 2 * o_rms and g_max <= 4 * o_max, f"{label}: GPU rms / max {g_rms:.3e} / {g_max:.3e} against the checker's {o_rms:.3e} / {o_max:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ROUTES))
def test_route_against_f64(product, oracle, case, reached):
    M, K, n, want, _ = ROUTES[case]
    x, w = operands(M, K, n, seed=M * 31 + K * 7 + n)
    y, trace = run_mulmat(product, w, x)
    y_orc, _ = run_mulmat(oracle, w, x, gpu=False)
    reached.update(trace)
    check_clean(y, y_orc, x, w, case)
    assert trace == want, f"{case}: launched {trace}, the case targets {want}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BATCHED))
def test_batched_and_strided_against_f64(product, oracle, case, reached):
    M, K, n, B, strided, want = BATCHED[case]
    x, w = operands(M, K, n, seed=M + K + n + B, B=B)
    y, trace = run_mulmat(product, w, x, strided=strided)
    y_orc, _ = run_mulmat(oracle, w, x, gpu=False, strided=strided)
    reached.update(trace)
    check_clean(y, y_orc, x, w, case)
    assert trace == want, f"{case}: launched {trace}, the case targets {want}"


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def plant_specials(x, w):
    """NaN (high payload) at x[n0, k0], NaN 0x7f800001 (payload in the low 16 bits only) at x[n1, k1], +inf at w[m0, k2] and -inf at w[m1, k3]
    over an x column with zeros (inf * 0), +-0 elsewhere.  Returns the rows and columns that must be non-finite."""
    n, K = x.shape
    M = w.shape[0]
    n0, n1 = 1 % n, (n - 1) if n > 2 else 0
    m0, m1 = 3 % M, M - 2
    k0, k1, k2, k3 = 5, K // 2 + 1, K - 3, K // 3
    x[n0, k0] = _f32(0x7FC12345)
    x[n1, k1] = _f32(0x7F800001)
    w[m0, k2] = np.inf
    w[m1, k3] = -np.inf
    x[:: 2, k3] = 0.0                                                  # inf * 0 = NaN in column m1, every other row
    x[-1, k3] = -0.0
    return {n0, n1}, {m0, m1}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ROUTES))
def test_route_special_values(product, oracle, case, reached):
    """NaN in a token row makes exactly that row NaN; an infinite weight makes exactly its column non-finite with the reference's signs and
    NaN positions (inf * 0, inf - inf); every other element stays finite and within the bound (padding masked by multiply-by-zero would
    leak NaN there).  Then a clean call on the SAME context gives the bits of a clean call on a fresh one (split-K partials, activation planes)."""
    M, K, n, want, want_special = ROUTES[case]
    x, w = operands(M, K, n, seed=M * 31 + K * 7 + n)
    xs, ws = x.copy(), w.copy()
    rows, colsx = plant_specials(xs, ws)
    ref = ieee_reference(xs, ws)
    ml = product
    ctx = ml.NewContext(4, False, False)
    try:
        y, trace = run_mulmat(ml, ws, xs, ctx=ctx)
        y_clean_same, _ = run_mulmat(ml, w, x, ctx=ctx)
    finally:
        ml.ReleaseContext(ctx)
    y_clean_fresh, _ = run_mulmat(ml, w, x)
    y_orc, _ = run_mulmat(oracle, ws, xs, gpu=False)
    reached.update(trace)
    special = ~np.isfinite(ref)
    # the checker agrees with the order-independent model
    assert np.array_equal(np.isnan(y_orc), np.isnan(ref)) and np.array_equal(np.isposinf(y_orc), np.isposinf(ref)) and np.array_equal(np.isneginf(y_orc), np.isneginf(ref))
    assert np.array_equal(np.isnan(y), np.isnan(ref)), f"{case}: NaN at {np.argwhere(np.isnan(y) != np.isnan(ref))[:5].tolist()} differs from the reference"
    assert np.array_equal(np.isposinf(y), np.isposinf(ref)) and np.array_equal(np.isneginf(y), np.isneginf(ref)), f"{case}: infinities differ from the reference"
    assert set(np.argwhere(special)[:, 0]) >= rows and set(np.argwhere(special)[:, 1]) >= colsx
    xf, wf = np.where(np.isfinite(xs), xs, 0), np.where(np.isfinite(ws), ws, 0)
    y64, scale = exact_product(xf, wf)
    ok = np.abs(y.astype(np.float64) - y64) <= BOUND_C * U * scale
    assert ok[~special].all(), f"{case}: {np.count_nonzero(~ok[~special])} finite elements outside the bound"
    assert np.array_equal(y_clean_same.view(np.uint32), y_clean_fresh.view(np.uint32)), f"{case}: a clean call after the NaN call differs from a fresh context"
    assert trace == (want_special or want), f"{case}: launched {trace}"


@pytest.mark.gpu
@pytest.mark.parametrize("tiny", [False, True], ids=["large", "large_tiny"])
@pytest.mark.parametrize("case", sorted(ROUTES))
def test_route_extreme_values(product, case, tiny, reached):
    """Large and tiny operands, on disjoint halves of K so that no element mixes them.  Row 0: |x| near FLT_MAX (first half) against weights
    small enough that no partial sum can overflow in any order; row 1 (n > 1): every term of column 0 positive and their sum past FLT_MAX -
    +inf in every order; with `tiny`, the last row (n > 2): x in [2^-149, 2^-110] (second half) against weights of 2^100 in column M - 1,
    products normal.  Expected: the reference's result - within the bound, +inf where it overflows.  Large values alone stay on the bf16-split
    GEMM (they are inside its exact range); tiny ones send it to the fp32 GEMM.  Then a clean call on the SAME context gives the bits of a
    clean call on a fresh one (activation planes and split-K partials of the large call left behind)."""
    M, K, n, want, want_special = ROUTES[case]
    tiny = tiny and n > 2
    x0, w0 = operands(M, K, n, seed=M * 31 + K * 7 + n)
    x, w = operands(M, K, n, seed=M * 3 + K + n * 5)
    r = np.random.default_rng(K + n)
    h = K // 2
    w[:, :] = (w / np.float32(4 * K)).astype(np.float32)
    x[0, :h] = (r.uniform(0.5, 1.0, h) * 1.5e38 * r.choice([-1, 1], h)).astype(np.float32)
    x[0, h:] = 0.0
    w[0, :h] = np.float32(4.0 / K)                                     # row 0: sum_k |x w| <= 3e38 < FLT_MAX
    w[0, h:] = 0.0
    if n > 1:
        x[1, :h] = np.float32(3.0e38)                                   # row 1, column 0: 6e38 in every order
        x[1, h:] = 0.0
    if tiny:
        x[-1, h:] = (np.ldexp(1.0, r.integers(-149, -109, K - h)) * r.choice([-1, 1], K - h)).astype(np.float32)
        w[M - 1, h:] = (np.float32(2.0 ** 100) * r.choice([-1, 1], K - h)).astype(np.float32)
    ml = product
    ctx = ml.NewContext(4, False, False)
    try:
        y, trace = run_mulmat(ml, w, x, ctx=ctx)
        y_clean_same, _ = run_mulmat(ml, w0, x0, ctx=ctx)
    finally:
        ml.ReleaseContext(ctx)
    y_clean_fresh, _ = run_mulmat(ml, w0, x0)
    reached.update(trace)
    y64, scale = exact_product(x, w)
    expect_inf = np.zeros(y64.shape, bool)
    if n > 1:
        expect_inf[1, 0] = True
    assert np.isposinf(y[expect_inf]).all(), f"{case}: an overflowing row did not give +inf"
    fin = ~expect_inf & (np.abs(y64) < 3.4e38)
    assert np.isfinite(y[fin]).all(), f"{case}: {np.count_nonzero(~np.isfinite(y[fin]))} elements overflowed that cannot in any order"
    bad = np.count_nonzero(~(np.abs(y[fin].astype(np.float64) - y64[fin]) <= BOUND_C * U * scale[fin]))
    assert bad == 0, f"{case}: {bad} elements outside the bound"
    assert np.array_equal(y_clean_same.view(np.uint32), y_clean_fresh.view(np.uint32)), f"{case}: a clean call after the large call differs from a fresh context"
    assert trace == ((want_special or want) if tiny else want), f"{case}: launched {trace}"


@pytest.fixture(scope="module")
def reached():
    return set()


@pytest.mark.gpu
def test_zz_every_node_path_instantiation_is_reached(reached):
    """Closing case: the instantiations this module's cases launched are exactly the node-path list written out from the dispatch
    (NODE_PATH_INSTANTIATIONS), minus EXEMPT."""
    if not reached:
        pytest.skip("no route case of this module ran in this session")
    assert set(EXEMPT) <= NODE_PATH_INSTANTIATIONS, f"exempt entries not in the list: {sorted(set(EXEMPT) - NODE_PATH_INSTANTIATIONS)}"
    expected = NODE_PATH_INSTANTIATIONS - set(EXEMPT)
    assert not (set(EXEMPT) & reached), f"exempt instantiations that ran: {sorted(set(EXEMPT) & reached)}"
    assert reached == expected, f"missing {sorted(expected - reached)}, not listed {sorted(reached - expected)}"
