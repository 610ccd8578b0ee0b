"""The cache probes of the fused plan: what the wq|wk|wv launch leaves in the KV cache and in q, against a float64 RoPE of a float64 product, element by
element - probe layers, reference, bound, two float32 evaluations, the mutants and the case matrix of tests/test_cache_probe_cpu.py and
tests/test_gpu_cache_probe.py.  Written from the mathematics of one LLaMA layer; numpy only; it shares no code with oracle/oracle.c or with the kernels
(the linear-map helper, the inputs and the numpy quantiser come from tests/weight_probe_ref.py).

WHAT IS COMPUTED (float64), row x at position t, H heads of hd channels, eps = fl32(1e-5):

    xn   = rms(x) g1                         rms(x)_c = x_c / sqrt(mean_c x_c^2 + eps)
    a^q, a^k, a^v = Wq xn, Wk xn, Wv xn      the raw products
    q, k = RoPE_t(a^q), RoPE_t(a^k)          pair (2i, 2i+1) of EVERY head turned by t theta_i, theta_i = 10000^(-2i / hd):
                                                 k_2i = a_2i cos - a_2i+1 sin,    k_2i+1 = a_2i sin + a_2i+1 cos
    cache K[slot][t][:] = k,  V[slot][t][:] = a^v        slot = layer - first layer of the stage, K and V alike; q goes to the attention

THE PROBES.  All zero w1 / w2 / w3; g1 = 1 + 0.1 N(0,1) (a gain left out or taken from a neighbour shows); every layer of a stage has its own seed.

    kv-sparse   wq = wo = 0,  wk[c, (c+1) mod d] = 2^(((c + L) mod 5) - 2),  wv[c, (c+3) mod d] = 2^(((c + L) mod 3) - 1)     (L = layer - first layer)
                One entry per row: the product is ONE term, exact in every summation order, through a K-split and through the three-plane bf16 split.  K shows
                the norm and RoPE alone - the sharp check of angle, position, sign and partner of every pair - and a slice or channel mix-up shows as a wrong
                shift (K is x shifted by 1, V by 3) or a wrong power of two.
    kv-dense    wq = wo = 0,  wk = Rk, wv = Rv dense N(0,1) / sqrt(d): the launch as it runs in a model.
    q           wq = R dense, wk = wv = 0, wo = 64 I.  q never leaves the device but through the attention, so the host first writes cache positions 0 .. P-1
                (P >= hd): K[t] = KEY_GAIN e_t and V[t] = e_t in every head for t < hd, zeros for hd <= t < P.  The call then feeds n rows at past = P; their
                own keys and values are exactly 0.  Key t < hd scores KEY_GAIN q_jht / sqrt(hd), every other visible key 0, so

                    x_out[j, h hd + c] = x + 64 p_jhc,   p_jhc = exp(KEY_GAIN q_jhc / sqrt(hd)) / Z_jh,   Z_jh = sum_c exp(..) + (P - hd) + (j + 1)

                Every element of q moves its own output element with sensitivity p (1 - p); the zero-score keys pin a common shift of a head's q.  The
                comparison is forward (x_out against x_out), nothing is inverted.

With wo = 0 (kv-*) and a zero FFN the stage's output equals its input BIT FOR BIT and a second layer sees the first one's input: the kv probes run on a
middle stage of two layers, so that the slot of the second layer shows.  The reference takes every weight as READ BACK from the device (block-int8:
fl32(d q)).

THE INPUTS.  weight_probe_ref.inputs: rows of N(0,1) times a power of two per row.  A call of n rows at `past` takes rows (past + i) mod len(X): the same row at
the same position in every call that holds it.

THE BOUND, element-wise, u = 2^-24, C = BOUND_C = 16 and DELTA = (C / 2 + 4) u = 12 u as derived in tests/weight_probe_ref.py.

  raw product a = W xn, bound b:
    dense    b = C u (|W| |xn|)          a float32 dot product in any order a kernel uses (weight_probe_ref)
               + DELTA |W xn|            the one rsqrt of the row is a common factor: it passes the linear map as a factor on the result
               + 3 u (|W| |xn|)          per element of xn: the two multiplies and a stored or re-rounded copy
    sparse   b = DELTA |w xn| + 3 u |w xn| + 2 u |w xn|
                                         one entry per row, so |W| |xn| = |W xn|; no summation error at all.  The last term is the product itself: a power
                                         of two times xn is exact on fp32 weights; read back from block-int8 the entry is fl32(d 127), and the scale-factored
                                         form rounds q xn and the product with d.  (Of the 3 u of xn only two are roundings there: five in all.)
  rotated pair (a0, a1) with raw bounds (b0, b1), c = cos, s = sin of the float64 angle:
    |k0' - k0| <=   |c| b0 + |s| b1                     the raw errors pushed through the rotation
                  + u (|c a0| + |s a1|)                 the raw value is a float32 in front of the rotation (half an ulp of each, both signs of the angle error: u)
                  + 1.5 u (|a0| + |a1|)                 another libm's cos / sin and the angle t theta_i in float64: the constant of tests/graph_ops_ref.py
                  + u / 2 |k0|                          the one final rounding (the rotation itself runs in float64)
    and the same with s and c exchanged for k1.
  V:  b + u / 2 |v|.
  q probe:  tests/attention_ref.py's bound with K and V as written: eps_j = max_t [(hd + 8) u KEY_GAIN |q_t| / sqrt(hd) + KEY_GAIN bq_t / sqrt(hd)] (the
    float32 score of a one-term product, plus what q_t itself may be off by - the rotated bound above with the dense raw bound), T_j = P + j + 1,
    B_jc = (expm1(2 eps_j) + (T_j + 16) u) p_jc, and |x_out - ref| <= (|wo| B_j)_c + 2 u |x_out|.

Sparse, combined: (DELTA + 5 u) (|c a0| + |s a1|) + u (|c a0| + |s a1|) + 1.5 u (|a0| + |a1|) + u / 2 |k0| - about 20 u of the pair's size, no term of it
fitted to a kernel.  tests/test_cache_probe_cpu.py holds two float32 evaluations inside (kv-sparse: at most half of it) and every mutant outside.

WHAT THE BOUND CANNOT SEE.  A pair whose angle is wrong by less than about 20 u radians (position 0 hides every angle mutant: cos = 1, sin = 0 - so every case
holds rows past position 0); a q error common to a head (softmax is shift-invariant but for the zero-score keys, which see it with weight (P - hd + j + 1) / Z);
anything in cache rows the call was not asked to write is seen bit for bit by the sentinel, not by the bound.
"""
import numpy as np

from weight_probe_ref import (U, BOUND_C, RMS_EPS, SHAPES as _WP_SHAPES, ROWS, ROWS_PAST, expected_route as _wp_expected_route, inputs as _wp_inputs, ff_size,
                              Lin, quantize_q8, delta_common, TENSOR_NAMES)

KEY_GAIN = 8.0
WO_GAIN = 64.0
CTX = 256
PAST = 7
KV_PROBES = ("kv-sparse", "kv-dense")
PROBES = KV_PROBES + ("q",)

HD_SHAPES = {
    "hd64": dict(vocab=2048, embd=1024, mult=256, heads=16),
    "hd32": dict(vocab=2048, embd=1024, mult=256, heads=32),
    "hd16": dict(vocab=515, embd=640, mult=32, heads=40),
}
SHAPES = dict(_WP_SHAPES, **HD_SHAPES)
HD_ROWS = (1, 3, 8, 9, 16, 17, 64, 65, 129, 193)
LONG_CTX = 2048
LONG_ROWS = (1, 4, 16, 64, 129)              # `small` at ctx = 2048, past = 2048 - n
_X_OF = {"hd64": "small", "hd32": "small", "hd16": "odd640"}      # weight_probe_ref.inputs depends on the width alone


def head_dim(shape):
    return SHAPES[shape]["embd"] // SHAPES[shape]["heads"]


def inputs(shape, rows):
    return _wp_inputs(_X_OF.get(shape, shape), rows)


def expected_route(shape, wtype, n, last=False):
    """weight_probe_ref.expected_route, extended by the head-dim shapes from the selectors of csrc/plan.hip.
    hd64 / hd32: `small` with more heads - no selector of a weight launch reads the head size but through hd % 4, hd % 32 and d % hd, all 0 here.
    hd16 (d = 640, F = 1728): block-int8 - hd % 32 keeps the dequantising GEMM out and F % 128 the plane kernel (q8b_shape_ok): n single steps behind the 2..4
    rows of the decode launches.  fp32 - d and F are multiples of 32 (prefill_mfma) but F is none of 128 (stream_shape_ok, b9s_shape_ok): wq|wk|wv and w1|w3 on
    the stream kernels up to 128 rows (K = d = 5 x 128), wo (K / 128 < 8: no K-split pair) and w2 (K = F) on the tile GEMM; beyond 128 rows no two-pass
    (stream_shape_ok) and no fused tile-GEMM epilogue (fewer tiles than CUs): plain tile GEMMs and k_rope_store."""
    if shape in ("hd64", "hd32"):
        return _wp_expected_route("small", wtype, n, last)
    if shape != "hd16":
        return _wp_expected_route(shape, wtype, n, last)
    if n == 1:
        return "Step", (), True
    if wtype == "q8":
        return ("Rows" if n <= 4 else "Q8Steps"), (), True
    if n <= 8:
        return "Rows", (), True
    if n <= 128:
        first = "k_stream_mm2" if n <= 16 else "k_stream_dma"
        return first + "+k_gemm", (first, "k_gemm_"), False
    return "k_gemm+k_rope_store", ("k_gemm_",), False


# ------------------------------------------------------------------------------------------------------------------------------------------
# probes
# ------------------------------------------------------------------------------------------------------------------------------------------
def probe_tensors(probe, shape, L=0, seed=23):
    """The fp32 tensors SetTensor gets for layer L of the stage (keys of weight_probe_ref.TENSOR_NAMES)."""
    kw = SHAPES[shape]
    d = kw["embd"]
    F = ff_size(d, kw["mult"])
    f = np.float32
    rng = np.random.default_rng(seed + 1000 * PROBES.index(probe) + 100 * L + d)
    gain = lambda: (1.0 + 0.1 * rng.standard_normal(d)).astype(f)                      # noqa: E731
    dense = lambda: rng.standard_normal((d, d), dtype=f) / f(np.sqrt(d))              # noqa: E731
    T = dict(g1=gain(), g2=gain(), wq=np.zeros((d, d), f), wk=np.zeros((d, d), f), wv=np.zeros((d, d), f), wo=np.zeros((d, d), f),
             w1=np.zeros((F, d), f), w3=np.zeros((F, d), f), w2=np.zeros((d, F), f))
    c = np.arange(d)
    if probe == "kv-sparse":
        T["wk"][c, (c + 1) % d] = 2.0 ** (((c + L) % 5) - 2)
        T["wv"][c, (c + 3) % d] = 2.0 ** (((c + L) % 3) - 1)
    elif probe == "kv-dense":
        T["wk"], T["wv"] = dense(), dense()
    elif probe == "q":
        T["wq"] = dense()
        T["wo"][c, c] = WO_GAIN
    else:
        raise ValueError(probe)
    return T


READ_BACK = {"kv-sparse": ("g1", "wk", "wv"), "kv-dense": ("g1", "wk", "wv"), "q": ("g1", "wq", "wo")}     # what the reference of a probe reads


def as_device(T, wtype):
    """The weights a device model holds for the tensors T (weight_probe_ref.as_device)."""
    if wtype == "f32":
        return dict(T)
    return {k: (quantize_q8(v)[2] if v.ndim == 2 and np.any(v) else v) for k, v in T.items()}


def sentinel(which, n):
    """What floats 0 .. n-1 of a cache hold before a call: finite, a function of the offset (a copied or shifted row shows), different for K and V, and far
    from anything a probe writes (>= 1024)."""
    off = np.arange(n, dtype=np.int64)
    return (1024.0 + ((off * 7 + 3 * which) % 8191) * 0.125).astype(np.float32)


def call_rows(T, n, past):
    """The rows of X (T of them) a call of n rows at `past` feeds."""
    return (past + np.arange(n)) % T


# ------------------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("k_pos+1", "q_pos+1", "no_past", "angle_next", "low_pair_neighbour", "sin_flip", "partner_swap", "head_wrap", "v_rotated", "kv_swapped", "row+1",
           "slot0", "two_pass_past", "pod0_pos", "extra_row")
KV_MUTANTS = tuple(m for m in MUTANTS if m not in ("q_pos+1", "pod0_pos"))             # (pod0_pos: the batched cases)
Q_MUTANTS = ("q_pos+1", "no_past", "angle_next", "low_pair_neighbour", "sin_flip", "partner_swap", "head_wrap", "two_pass_past")


def _rms_gain(x, g):
    r = 1.0 / np.sqrt(np.mean(x * x, axis=1) + RMS_EPS)
    return x * r[:, None] * g[None, :]


def raw_product(W, name, xn):
    """-> (a = W xn, b = its bound), [n][d] each."""
    L = _lin(W, name)
    (a,), (aa,) = L.mm([xn], [xn])
    d = xn.shape[1]
    if L.dense:
        return a, (BOUND_C + 3) * U * aa + delta_common(d) * np.abs(a)
    assert L.zero or L.terms == 1, f"{name}: a sparse probe matrix has one entry per row"
    return a, (delta_common(d) + 5 * U) * np.abs(a)


def _lin(W, name):
    cache = W.setdefault("_lin", {})
    if name not in cache:
        cache[name] = Lin(W[name])
    return cache[name]


def angles(pos, hd, H, mut=None):
    """[n][H][hd / 2]: the angle of pair i of head h of the row at position pos."""
    theta = 10000.0 ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    pos = np.asarray(pos, dtype=np.float64)
    ang = np.repeat((pos[:, None] * theta[None, :])[:, None, :], H, axis=1)
    if mut == "angle_next":                    # pair i takes pair i + 1's angle (the last one the first's)
        ang = np.roll(ang, -1, axis=2)
    elif mut == "low_pair_neighbour":          # only the lowest-frequency pair takes its neighbour's
        ang[:, :, -1] = ang[:, :, -2]
    elif mut == "head_wrap":                   # table index (e mod 2 hd) / 2: the odd heads run into the next position's entries
        ang[:, 1::2, :] = ((pos + 1)[:, None] * theta[None, :])[:, None, :]
    return ang


def rotate(a, b, ang, mut=None):
    """a, b [n][d] raw values and bounds, ang [n][H][hd / 2] -> (rotated, its bound) [n][d]."""
    n, d = a.shape
    H, half = ang.shape[1], ang.shape[2]
    a4, b4 = a.reshape(n, H, half, 2), b.reshape(n, H, half, 2)
    a0, a1, b0, b1 = a4[..., 0], a4[..., 1], b4[..., 0], b4[..., 1]
    if mut == "partner_swap":
        a0, a1 = a1, a0
    c, s = np.cos(ang), np.sin(ang)
    if mut == "sin_flip":
        s = -s
    out, bound = np.empty_like(a4), np.empty_like(a4)
    out[..., 0] = a0 * c - a1 * s
    out[..., 1] = a0 * s + a1 * c
    lib = 1.5 * U * (np.abs(a0) + np.abs(a1))
    ac, as_ = np.abs(c), np.abs(s)
    bound[..., 0] = ac * b0 + as_ * b1 + U * (ac * np.abs(a0) + as_ * np.abs(a1)) + lib + U / 2 * np.abs(out[..., 0])
    bound[..., 1] = as_ * b0 + ac * b1 + U * (as_ * np.abs(a0) + ac * np.abs(a1)) + lib + U / 2 * np.abs(out[..., 1])
    return out.reshape(n, d), bound.reshape(n, d)


def rot_positions(pos, mut):
    """The position each row is rotated with."""
    pos = np.asarray(pos, dtype=np.int64)
    n = len(pos)
    if mut == "no_past":                       # the row index without `past` (Rope mode 0 and mode 1 mixed up)
        return np.arange(n)
    if mut == "two_pass_past":                 # the second half of a two-pass call restarts at `past`
        b0 = (n + 1) // 2
        return np.concatenate([pos[:b0], pos[0] + np.arange(n - b0)])
    return pos


def kv_reference(layers, x, pos, H, mut=None):
    """The cache rows a call writes: layers = the stage's weight dicts in slot order, x [n][d] float32 rows at the positions pos.
    -> dict(K, V, bK, bV [S][n][d]; row [n] the cache row of each input row; slot [S] the slot each layer writes)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    pos = np.asarray(pos, dtype=np.int64)
    n, d = x.shape
    hd = d // H
    rp = rot_positions(pos, mut) + (1 if mut == "k_pos+1" else 0)
    ang = angles(rp, hd, H, mut)
    out = dict(K=[], V=[], bK=[], bV=[])
    for W in layers:
        xn = _rms_gain(x, W["g1"].astype(np.float64))
        ak, bk = raw_product(W, "wk", xn)
        av, bv = raw_product(W, "wv", xn)
        if mut == "kv_swapped":
            ak, bk, av, bv = av, bv, ak, bk
        K, bK = rotate(ak, bk, ang, mut)
        V, bV = av, bv + U / 2 * np.abs(av)
        if mut == "v_rotated":
            V = rotate(av, bv, ang)[0]
        for k, v in zip(("K", "V", "bK", "bV"), (K, V, bK, bV)):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out["row"] = pos + (1 if mut == "row+1" else 0)
    if mut == "extra_row":                     # one more row than asked for: the last row's values again behind it - only the sentinel sees it
        out = {k: np.concatenate([v, v[:, -1:]], axis=1) for k, v in out.items() if k != "row"} | dict(row=np.append(out["row"], pos[-1] + 1))
    out["slot"] = np.zeros(len(layers), dtype=np.int64) if mut == "slot0" else np.arange(len(layers))
    return out


def cache_images(res, S, ctx, d, base=None):
    """(K, V) float32 [S][ctx][d]: the sentinel (or `base`, a pair of images), then the rows of `res` where it puts them - flat addressing, as a kernel would:
    a row past the slot's end lands in the next slot, one past the cache's end is dropped (the reference of an out-of-bounds write is not to run it)."""
    imgs = []
    for which, key in enumerate(("K", "V")):
        img = (sentinel(which, S * ctx * d) if base is None else np.array(base[which], dtype=np.float32).ravel())
        for s in range(len(res["slot"])):
            for i, row in enumerate(res["row"]):
                off = (int(res["slot"][s]) * ctx + int(row)) * d
                if 0 <= off and off + d <= img.size:
                    img[off:off + d] = res[key][s][i].astype(np.float32)
        imgs.append(img.reshape(S, ctx, d))
    return imgs


def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max()) if err.size else 0.0


def check_cache(K_img, V_img, ref, pos, base=None):
    """K_img, V_img [S][ctx][d] as read from a cache that held the sentinel (or `base`); ref = kv_reference of the call (clean), pos its positions.
    -> dict(rK, rV: the worst error / bound over the rows the call writes, all slots; stray: how many floats of every other row differ from what the cache
    held before, bit for bit)."""
    S, ctx, d = K_img.shape
    pos = np.asarray(pos, dtype=np.int64)
    out = dict(stray=0)
    written = np.zeros(ctx, dtype=bool)
    written[pos] = True
    for which, (img, key, bkey) in enumerate(((K_img, "K", "bK"), (V_img, "V", "bV"))):
        img = np.ascontiguousarray(img, dtype=np.float32)
        out["r" + key] = max([_ratio(img[s][pos], ref[key][s], ref[bkey][s]) for s in range(S)], default=0.0) if len(pos) else 0.0
        before = (sentinel(which, S * ctx * d) if base is None else np.ascontiguousarray(base[which], dtype=np.float32).ravel()).reshape(S, ctx, d)
        out["stray"] += int(np.count_nonzero(img[:, ~written].view(np.uint32) != before[:, ~written].view(np.uint32)))
    return out


def q_prefill(H, hd, P):
    """The K and V rows 0 .. P-1 the host writes in front of a q call: [P][d] each."""
    d = H * hd
    K, V = np.zeros((P, d), dtype=np.float32), np.zeros((P, d), dtype=np.float32)
    t = np.arange(hd)
    for h in range(H):
        K[t, h * hd + t] = KEY_GAIN
        V[t, h * hd + t] = 1.0
    return K, V


def q_reference(W, x, P, H, mut=None):
    """x_out of the q probe for the rows x [n][d] fed at past = P behind q_prefill.  -> dict(out, bound, attn: the (wo attn) term [n][d])."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, d = x.shape
    hd = d // H
    assert P >= hd
    pos = P + np.arange(n)
    rp = rot_positions(pos, mut) + (1 if mut == "q_pos+1" else 0)
    xn = _rms_gain(x, W["g1"].astype(np.float64))
    a, b = raw_product(W, "wq", xn)
    q, bq = rotate(a, b, angles(rp, hd, H, mut), mut)
    scale = 1.0 / np.sqrt(hd)
    s = (KEY_GAIN * scale * q).reshape(n, H, hd)
    e = np.exp(s)
    Tj = (P + np.arange(1, n + 1)).astype(np.float64)
    Z = e.sum(axis=2) + (Tj - hd)[:, None]                       # the zero-score keys: P - hd written ones and the call's own j + 1
    p = e / Z[:, :, None]
    eps = ((hd + 8) * U * KEY_GAIN * scale * np.abs(q) + KEY_GAIN * scale * bq).reshape(n, H, hd).max(axis=2)
    B = (np.expm1(2 * eps) + ((Tj + 16) * U)[:, None])[:, :, None] * p
    Lo = _lin(W, "wo")
    (Y,), (bY,) = Lo.mm([p.reshape(n, d)], [B.reshape(n, d)])
    out = x + Y
    return dict(out=out, bound=bY + 2 * U * np.abs(out), attn=Y)


def ratio(y, ref):
    return _ratio(y, ref["out"], ref["bound"])


# ------------------------------------------------------------------------------------------------------------------------------------------
# float32 evaluations
# ------------------------------------------------------------------------------------------------------------------------------------------
def _mm32(z, w, order, Q=None):
    """z [n][K] x w [M][K] in float32.  order 0: one BLAS call.  order 1: 32-wide K blocks summed from the LAST to the first; with Q = (q, d) the block-int8
    matrix in the scale-factored form sum_b d_b (sum_k q_k z_k)."""
    f = np.float32
    z = np.ascontiguousarray(z, dtype=f)
    if order == 0:
        return z @ np.ascontiguousarray(w, dtype=f).T
    src = Q[0].astype(f) if Q is not None else np.asarray(w, dtype=f)
    acc = np.zeros((z.shape[0], src.shape[0]), dtype=f)
    for b in reversed(range(z.shape[1] // 32)):
        part = z[:, 32 * b:32 * b + 32] @ src[:, 32 * b:32 * b + 32].T
        acc += part * Q[1][None, :, b] if Q is not None else part
    return acc


def _rms32(x, g, order):
    f = np.float32
    sq = x * x
    if order == 0:
        ms = np.mean(sq, axis=1, dtype=f)
    else:                                       # 64 interleaved partial sums, then those pairwise - the shape of a wave reduction
        part = sq.reshape(x.shape[0], -1, 64).sum(axis=1, dtype=f)
        ms = part.sum(axis=1, dtype=f) / f(x.shape[1])
    return x * (f(1) / np.sqrt(ms + f(RMS_EPS)))[:, None] * g.astype(f)[None, :]


def _rope32(a, pos, H):
    f = np.float32
    n, d = a.shape
    hd = d // H
    ang = angles(pos, hd, H)                    # the angles and their cos / sin in float64, then cast (the kernels read a float64 table)
    c, s = np.cos(ang).astype(f), np.sin(ang).astype(f)
    a4 = a.reshape(n, H, hd // 2, 2)
    out = np.empty_like(a4)
    out[..., 0] = a4[..., 0] * c - a4[..., 1] * s
    out[..., 1] = a4[..., 0] * s + a4[..., 1] * c
    return out.reshape(n, d)


def kv_f32(layers, x, pos, H, order=0, Q=None):
    """The cache rows in plain float32.  order 0: textbook; 1: another summation order for the sum of squares and the product.  Q: per layer {name: (q, d)}.
    -> dict(K, V [S][n][d], row, slot) for cache_images."""
    x = np.asarray(x, dtype=np.float32)
    K, V = [], []
    for i, W in enumerate(layers):
        xn = _rms32(x, W["g1"], order)
        Qi = (Q[i] if Q else {})
        K.append(_rope32(_mm32(xn, W["wk"], order, Qi.get("wk")), pos, H))
        V.append(_mm32(xn, W["wv"], order, Qi.get("wv")))
    return dict(K=np.stack(K), V=np.stack(V), row=np.asarray(pos, dtype=np.int64), slot=np.arange(len(layers)))


def q_f32(W, x, P, H, order=0, Q=None):
    """x_out of the q probe in plain float32: the scores against every key of the cache, a softmax over them, P V, wo, the residual."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    n, d = x.shape
    hd = d // H
    Q = Q or {}
    q = _rope32(_mm32(_rms32(x, W["g1"], order), W["wq"], order, Q.get("wq")), P + np.arange(n), H).reshape(n, H, hd)
    Kp, Vp = q_prefill(H, hd, P)
    Kc = np.concatenate([Kp, np.zeros((n, d), f)]).reshape(P + n, H, hd)
    Vc = np.concatenate([Vp, np.zeros((n, d), f)]).reshape(P + n, H, hd)
    vis = np.arange(P + n)[None, :] <= (P + np.arange(n))[:, None]
    attn = np.zeros((n, H, hd), dtype=f)
    for h in range(H):
        S = (q[:, h] @ Kc[:, h].T) * f(1.0 / np.sqrt(hd))
        S = np.where(vis, S, f(-np.inf))
        if order == 1:
            S, Vh = S[:, ::-1], Vc[::-1, h]
        else:
            Vh = Vc[:, h]
        e = np.exp(S - S.max(axis=1, keepdims=True))
        attn[:, h] = (e / e.sum(axis=1, dtype=f)[:, None]) @ Vh
    return (x + _mm32(attn.reshape(n, d), W["wo"], order, Q.get("wo"))).astype(np.float64)
