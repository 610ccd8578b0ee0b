"""The weight probes of the fused plan: probe layers, their float64 reference, the element-wise bound, two float32 evaluations, the mutants and the case
matrix of tests/test_weight_probe_cpu.py and tests/test_gpu_weight_probe.py.  Written from the mathematics of one LLaMA layer; it shares no code with
oracle/oracle.c or with the kernels.

THE LAYER (float64), T_j = j + 1 visible rows, eps = fl32(1e-5):

    xn1 = rms(x) g1               rms(x)_c = x_c / sqrt(mean_c x_c^2 + eps)
    v_t = Wv xn1_t,  attn_j = softmax-weighted mean of v_t, t <= j        (every probe has wq = wk = 0: the scores are exactly 0, the weights 1 / T_j)
    h   = x + Wo attn
    xn2 = rms(h) g2
    g   = silu(W1 xn2) (W3 xn2)
    out = h + W2 g
    logits (last stage, last row) = Wout (rms(out) norm)

THE PROBES.  R* is dense N(0,1) / sqrt(K) from a seeded generator; the norm gains are 1 + 0.1 N(0,1), so a gain that is left out or taken from a
neighbour shows; I z and 0 z are exact in every summation order.  "fold": W2[c, j] = 1 where j mod d == c.  "spread": W[j, j mod d] = gain.

    wv    wq = wk = 0, wv = R, wo = I, FFN 0         x_out_j = x_j + mean_{t <= j} R xn1_t          the third slice of wq|wk|wv and its cache append
    wo    wq = wk = 0, wv = I, wo = R, FFN 0         x_out_j = x_j + R mean_{t <= j} xn1_t
    w13   attention 0, w1 = R1, w3 = R3, w2 = fold   x_out_c = x_c + sum_{j = c mod d} g_j          every one of the F rows of the pair launch
    w2    attention 0, w1 = 1.5 spread, w3 = -0.75 spread, w2 = R        x_out = x + R g,  g_j = silu(1.5 xn2_c) (-0.75 xn2_c)
    head  layer matrices 0, norm = 1 + 0.1 N, output = R (V x d)         logits of the last row = R (rms(x) norm)

The reference takes every weight as READ BACK from the device (block-int8 models: fl32(d q)) and multiplies with whatever values it finds; matrices of at
most a few entries per row are multiplied entry by entry, the dense ones in float64 BLAS.  wq = wk = 0 is required (asserted), so is h = x exactly where the
FFN is probed.

THE INPUTS.  Rows of N(0,1) times a power of two in 2^-3 .. 2^3 per row: the rows and their rms differ, so a row mix-up shows.  One X per shape; a call of n
rows at `past` takes rows past .. past + n - 1, and - the layer being causal - its reference is those rows of the one reference of X.

THE BOUND, element-wise, u = 2^-24, C = BOUND_C = 16 (the constant of tests/test_gpu_matmul_routes.py, with its reasoning: a float32 dot product of K
terms in any order errs by at most K u sum|w z| in the worst case and by a few u sum|w z| in every order a kernel uses; 16 holds every MulMat route there):

    |out - ref| <=   C u (|W| |z|)                 the probed product, z its float64 input
                   + |W| dz                        what the kernel's own z may be off by (below)
                   + (terms + 2) u sum|w z|        a pass-through product (I, fold, spread: `terms` entries per row; read back from int8 they are not exactly 1)
                   + 2 u |out|                     residual add and final rounding

dz, term by term:

  RMSNorm gain input xn = x r g, r = 1 / sqrt(mean x^2 + eps).
    r is ONE number per row, so its error is common to the row: xn' = xn (1 + delta) with |delta| <= DELTA = (C / 2 + 4) u = 12 u:
        the sum of d squares is a float32 dot product of the row with itself and is counted like every other one here: C u sum x^2 (its terms are all
        positive, so that is C u relative), halved by the square root: C / 2.  (The any-order worst case, d u, would be 2048 u at d = 4096: one term of
        the bound would then outweigh the probed product's and hide what the probe is there to show.)
        the division by d (1/2 after the root), the added eps (1/2), the root (1) and the reciprocal or a 2-ulp rsqrt (2): 4.
    A common factor passes a linear map as the same factor on the RESULT: it costs delta |W xn|, not delta |W| |xn| - which is what keeps the bound
    sharp (|W xn| is sqrt(K) terms large, |W| |xn| K terms).  Where rows are mixed (the attention mean) the factors differ per row and the cost is
    DELTA mean_t |W xn_t|; behind silu it is DELTA |W2 e| with e = d g / d ln(scale of xn2) = silu'(a) a b + silu(a) b.
    Per element: the two multiplies and one for a stored or re-rounded copy: 3 u |xn|.

  Uniform attention (scores exactly 0, p_t = 1 / T_j): tests/attention_ref.py's (T_j + 16) u sum_t p_t |v_t| with eps = 0, plus the mean of v's own bound.

  g = silu(a) b:  |dg| <= |silu'(a)| |b| da + |silu(a)| db + (|a| + 8) u |g|
    da, db: the bounds of the two products.  exp(-a) evaluated in float32: the rounded argument moves it by |a| u relative, the function itself 3 u, and
    silu depends on it with a factor exp(-a) / (1 + exp(-a)) <= 1; the addition 1, the division 2 (a fast division), the product with b 1, one more for a
    stored copy: (|a| + 8) u |g|.  First order, as everywhere here.

No constant was fitted to a kernel.  What the bound cannot see: dropping only the LOWEST bf16 plane of an activation row is 2^-16 relative per term, about
sqrt(K) 2^-17 sum-wise - below 16 u K at every K here.  The middle plane (2^-8 per term) is seen (tests/test_weight_probe_cpu.py).
"""
import numpy as np

U = 2.0 ** -24
BOUND_C = 16.0
RMS_EPS = float(np.float32(1e-5))
A_GAIN, B_GAIN = 1.5, -0.75
CTX = 256
PAST = 7
LAYER_PROBES = ("wv", "wo", "w13", "w2")
PROBES = LAYER_PROBES + ("head",)

# names follow tests/eval_route_cases.py; "7Blayer": the 7B layer shape as one layer, vocabulary cut to 2048 like the 65B layer's
SHAPES = {
    "small": dict(vocab=2048, embd=1024, mult=256, heads=8),
    "odd640": dict(vocab=515, embd=640, mult=8, heads=5),
    "odd640m32": dict(vocab=515, embd=640, mult=32, heads=5),
    "7Blayer": dict(vocab=2048, embd=4096, mult=256, heads=32),
    "65Blayer": dict(vocab=2048, embd=8192, mult=256, heads=64),
}
# (shape, weight type) -> row counts at past = 0: both sides of every selector edge
ROWS = {
    ("small", "f32"): (1, 2, 4, 5, 8, 9, 16, 17, 48, 49, 64, 65, 128, 129, 192, 193),
    ("small", "q8"): (1, 2, 4, 5, 16, 64, 65, 88, 89, 129),
    ("odd640", "f32"): (1, 3, 8, 9, 40),
    ("odd640m32", "q8"): (1, 3, 8, 9, 40, 130),
    ("7Blayer", "f32"): (1, 4, 16, 64, 128),
    ("7Blayer", "q8"): (1, 4, 16, 89),
    ("65Blayer", "f32"): (5, 8),
}
# one row count per route, behind PAST unchecked rows
ROWS_PAST = {
    ("small", "f32"): (1, 4, 16, 48, 64, 129, 193),
    ("small", "q8"): (1, 4, 16, 65, 89),
    ("odd640", "f32"): (1, 8, 9, 40),
    ("odd640m32", "q8"): (1, 3, 8, 40, 130),
    ("7Blayer", "f32"): (1, 4, 16, 64, 128),
    ("7Blayer", "q8"): (1, 4, 16, 89),
    ("65Blayer", "f32"): (8,),
}
PROBES_OF = {"65Blayer": ("wv", "w13", "w2")}     # the only shape that reaches k_skinny: the launches with a folded norm, and w2


def probes_of(shape):
    return PROBES_OF.get(shape, PROBES)


def ff_size(d, mult):
    return ((2 * (4 * d) // 3 + mult - 1) // mult) * mult


def total_rows(shape, wtype):
    return max(max(ROWS[shape, wtype]), PAST + max(ROWS_PAST[shape, wtype]))


def expected_route(shape, wtype, n, last=False):
    """-> (family name for the report, the k_stream_ / k_gemm_ / k_gemv_cols names the trace must show and no others, quiet).  quiet: a route whose GEMV
    launches the trace does not name - it must show no such entry and the per-query attention.  last: a last stage (the `head` probe) - the odd
    vocabulary of 515 rows has no gemv_rows launch, so 2..8 fp32 rows go to the stream and column kernels there and to Rows on a middle stage, and
    2..4 block-int8 rows to n single steps."""
    if shape == "65Blayer":
        return "Skinny", (), True
    if shape == "odd640":
        if n == 1:
            return "Step", (), True
        if n <= 8 and not last:
            return "Rows", (), True
        first = "k_stream_mm2" if n <= 16 else "k_stream_dma" if n <= 128 else "k_gemm_glds"
        return first + "+k_gemv_cols", (first, "k_gemv_cols"), False
    if shape == "odd640m32":
        if n <= 8:
            return ("Step" if n == 1 else "Rows" if n <= 4 and not last else "Q8Steps"), (), True
        return ("k_gemm_q8", ("k_gemm_q8",), False) if n <= 64 else ("k_gemm_q8b3+k_gemm_q8", ("k_gemm_q8b3", "k_gemm_q8"), False)
    if wtype == "q8":
        if n <= 4:
            return ("Step" if n == 1 else "Rows"), (), True
        if n <= 88:
            return ("k_stream_q8b" if n <= 64 else "k_stream_q8b/two-pass"), ("k_stream_q8b",), False
        return "k_gemm_q8b3", ("k_gemm_q8b3",), False
    if n <= 8:
        return ("Step" if n == 1 else "Rows"), (), True
    if n <= 16:
        return "k_stream_mm2", ("k_stream_mm2",), False
    if 49 <= n <= 64:
        return "k_stream_b9", ("k_stream_b9",), False
    if n <= 192:
        return ("k_stream_dma" if n <= 128 else "k_stream_dma/two-pass"), ("k_stream_dma",), False
    return "k_gemm", ("k_gemm_",), False


# ------------------------------------------------------------------------------------------------------------------------------------------
# probes and inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
TENSOR_NAMES = dict(g1="attention_norm.weight", g2="ffn_norm.weight", wq="attention.wq.weight", wk="attention.wk.weight", wv="attention.wv.weight",
                    wo="attention.wo.weight", w1="feed_forward.w1.weight", w2="feed_forward.w2.weight", w3="feed_forward.w3.weight")
MATRICES = ("wq", "wk", "wv", "wo", "w1", "w2", "w3")
ZERO = {"wv": ("wq", "wk", "w1", "w2", "w3"), "wo": ("wq", "wk", "w1", "w2", "w3"), "w13": ("wq", "wk", "wv", "wo"), "w2": ("wq", "wk", "wv", "wo"),
        "head": MATRICES}


def inputs(shape, rows, seed=11):
    d = SHAPES[shape]["embd"]
    rng = np.random.default_rng(seed + d)
    X = rng.standard_normal((rows, d)) * (2.0 ** rng.integers(-3, 4, rows))[:, None]
    return X.astype(np.float32)


def probe_tensors(probe, shape, seed=5):
    """The fp32 tensors SetTensor gets: keys of TENSOR_NAMES, and for `head` also norm, output."""
    kw = SHAPES[shape]
    d, V = kw["embd"], kw["vocab"]
    F = ff_size(d, kw["mult"])
    f = np.float32
    rng = np.random.default_rng(seed + 1000 * PROBES.index(probe) + d)
    gain = lambda: (1.0 + 0.1 * rng.standard_normal(d)).astype(f)                      # noqa: E731
    dense = lambda m, k: rng.standard_normal((m, k), dtype=f) / f(np.sqrt(k))          # noqa: E731
    T = dict(g1=gain(), g2=gain(), wq=np.zeros((d, d), f), wk=np.zeros((d, d), f), wv=np.zeros((d, d), f), wo=np.zeros((d, d), f),
             w1=np.zeros((F, d), f), w3=np.zeros((F, d), f), w2=np.zeros((d, F), f))
    j = np.arange(F)
    if probe == "wv":
        T["wv"], T["wo"] = dense(d, d), np.eye(d, dtype=f)
    elif probe == "wo":
        T["wv"], T["wo"] = np.eye(d, dtype=f), dense(d, d)
    elif probe == "w13":
        T["w1"], T["w3"] = dense(F, d), dense(F, d)
        T["w2"][j % d, j] = 1
    elif probe == "w2":
        T["w1"][j, j % d], T["w3"][j, j % d] = A_GAIN, B_GAIN
        T["w2"] = dense(d, F)
    elif probe == "head":
        T["norm"], T["output"] = gain(), dense(V, d)
    else:
        raise ValueError(probe)
    return T


def quantize_q8(w):
    """numpy restatement of the block-int8 rule (csrc/kernels_q8.h): per 32 weights d = fl32(max|w| / 127), q = clamp(rint(fl32(w / d)), -127, 127)
    (d = 0: q = 0), w' = fl32(d q); a block that holds a NaN or an infinity: d = NaN, q = 0.  -> (q int8, d float32 [.., K / 32], w' float32)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = w.reshape(-1, 32)
    f = np.float32
    with np.errstate(all="ignore"):
        bad = ~np.all(np.isfinite(b), axis=1)
        m = np.max(np.abs(np.where(bad[:, None], f(0), b)), axis=1)
        d = (m / f(127)).astype(f)
        q = np.where(d[:, None] > 0, np.rint((b / np.where(d > 0, d, f(1))[:, None]).astype(f)), f(0))
        q = np.where(bad[:, None], f(0), np.clip(q, -127, 127)).astype(np.int8)      # (an int8 0 has no sign: rint(-0.5) = -0 dequantises to +0)
        d = np.where(bad, f(np.nan), d).astype(f)
        deq = (d[:, None] * q.astype(f)).astype(f)
    return q.reshape(w.shape), d.reshape(w.shape[:-1] + (w.shape[-1] // 32,)), deq.reshape(w.shape)


def as_device(T, wtype):
    """The weights a device model holds for the tensors T: fp32 as set; block-int8: every matrix (the lm_head too) through the quantiser, norm vectors fp32."""
    if wtype == "f32":
        return dict(T)
    return {k: (quantize_q8(v)[2] if v.ndim == 2 and np.any(v) else v) for k, v in T.items()}


# ------------------------------------------------------------------------------------------------------------------------------------------
# linear maps
# ------------------------------------------------------------------------------------------------------------------------------------------
class Lin:
    """y = W z for a float32 matrix W [M][K] as read back, z [n][K] float64.  At most 4 max(M, K) entries: kept as (row, column, value) and multiplied
    entry by entry; else dense, in float64, in row chunks (a 65B w1 is 1.4 GB as float64)."""

    def __init__(self, W):
        W = np.asarray(W, dtype=np.float32)
        assert W.ndim == 2 and np.all(np.isfinite(W))
        self.M, self.K = W.shape
        nz = int(np.count_nonzero(W))
        self.zero, self.dense = nz == 0, nz > 4 * max(W.shape)
        if self.dense:
            self.W, self.terms = W, self.K
        else:
            self.r, self.c = np.nonzero(W)
            self.v = W[self.r, self.c].astype(np.float64)
            self.terms = int(np.bincount(self.r, minlength=1).max()) if nz else 0
        # the constant of C u |W| |z|: the probed (dense) product, or a pass-through one
        self.C = BOUND_C if self.dense else self.terms + 2

    def mm(self, signed=(), absolute=()):
        """-> ([W z for z in signed], [|W| z for z in absolute]) in one pass over W."""
        n_s = len(signed)
        zs = [np.asarray(z, dtype=np.float64) for z in signed] + [np.abs(np.asarray(z, dtype=np.float64)) for z in absolute]
        # the last few results are kept by the bytes of their operands: the mutants of one case repeat most products of each other (callers copy before
        # they change a result), and a pass over a 65B matrix costs seconds
        memo = self.__dict__.setdefault("_memo", {})
        key = (n_s,) + tuple(hash(np.ascontiguousarray(z).tobytes()) for z in zs)
        if key in memo:
            outs = memo[key]
            return outs[:n_s], outs[n_s:]
        outs = [np.zeros((z.shape[0], self.M)) for z in zs]
        if self.dense:
            for i in range(0, self.M, 2048):
                Wc = self.W[i:i + 2048].astype(np.float64).T
                Wa = np.abs(Wc) if len(zs) > n_s else None
                for k, z in enumerate(zs):
                    outs[k][:, i:i + 2048] = z @ (Wc if k < n_s else Wa)
        elif not self.zero:
            for k, z in enumerate(zs):
                np.add.at(outs[k].T, self.r, (z[:, self.c] * (self.v if k < n_s else np.abs(self.v))[None, :]).T)
        if sum(o.size for o in outs) <= 1 << 20:                 # (only small results: a handful of rows)
            while len(memo) >= 6:
                memo.pop(next(iter(memo)))
            memo[key] = outs
        return outs[:n_s], outs[n_s:]

    def row(self, m):
        """row m of W as float64 [K]"""
        if self.dense:
            return self.W[m].astype(np.float64)
        out = np.zeros(self.K)
        sel = self.r == m
        out[self.c[sel]] = self.v[sel]
        return out


def lin_of(W, name):
    """The Lin of W[name], built once per weight dict (kept under W["_lin"])."""
    cache = W.setdefault("_lin", {})
    if name not in cache:
        cache[name] = Lin(W[name])
    return cache[name]


def split3_mid(z):
    """The middle bf16 plane of fl32(z): bits 8..15 of the significand (csrc/kernels_common.h split3, restated), as float64."""
    a = np.asarray(z, dtype=np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = a - hi
    return (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the reference, with its bound and - for tests/test_weight_probe_cpu.py - the mutants
# ------------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("block_dropped", "neighbour_scale", "pair_swapped", "gamma_float4", "residual_missing", "residual_twice", "tile_row_shift", "v_late", "mid_plane")


def mutants_of(probe, wtype):
    """The mutants that exist on a probe: the neighbour's scale on block-int8 weights, the w1 / w3 exchange where both are dense, a residual where there
    is one, the late V row where the cache holds something."""
    out = ["block_dropped", "gamma_float4", "tile_row_shift", "mid_plane"]
    if wtype == "q8":
        out.append("neighbour_scale")
    if probe == "w13":
        out.append("pair_swapped")
    if probe != "head":
        out += ["residual_missing", "residual_twice"]
    if probe in ("wv", "wo"):
        out.append("v_late")
    return out


def delta_common(d):
    """DELTA of the module docstring; the same at every d: the sum of squares is counted with the product's constant, not with its term count."""
    return (BOUND_C / 2 + 4) * U


def _rms_gain(x, g):
    r = 1.0 / np.sqrt(np.mean(x * x, axis=1) + RMS_EPS)
    return x * r[:, None] * g[None, :]


def _silu(a):
    return a / (1.0 + np.exp(-a))


def _dsilu(a):
    s = 1.0 / (1.0 + np.exp(-a))
    return s * (1.0 + a * (1.0 - s))


def _cummean(v):
    return np.cumsum(v, axis=0) / np.arange(1, v.shape[0] + 1, dtype=np.float64)[:, None]


class _Mut:
    """One mutant and where it strikes: batch row r (and r + 1), output row m of the probed matrix, 32-column block b, output column c."""

    def __init__(self, name, r, m=3, b=1, c=6):
        self.name, self.r, self.m, self.b, self.c = name, r, m, b, c

    def norm(self, xn, x, g, probed):
        if probed and self.name == "gamma_float4":             # gamma left out of one float4 of one row
            xn = xn.copy()
            xn[self.r, 8:12] /= g[8:12]
        return xn

    def product(self, P, L, z, probed):
        """P = W z of the probed product"""
        if not probed:
            return P
        P = P.copy()
        blk = slice(32 * self.b, 32 * self.b + 32)
        if self.name == "block_dropped":
            P[self.r, self.m] -= L.row(self.m)[blk] @ z[self.r, blk]
        elif self.name == "neighbour_scale":                     # block b of row m multiplied by block b + 1's scale: d = max|w'| / 127 of the read-back block
            w = L.row(self.m)
            d0, d1 = np.abs(w[blk]).max(), np.abs(w[32 * self.b + 32:32 * self.b + 64]).max()
            assert d0 > 0 and d1 > 0 and d0 != d1
            P[self.r, self.m] += (d1 / d0 - 1.0) * (w[blk] @ z[self.r, blk])
        elif self.name == "tile_row_shift":                      # row r of a 16-row tile takes row r + 1's sums
            P[self.r] = P[self.r + 1]
        return P

    def operand(self, z, probed):
        if probed and self.name == "mid_plane":                  # the middle bf16 plane of one activation row dropped
            z = z.copy()
            z[self.r] -= split3_mid(z[self.r])
        return z


def reference(probe, W, X, mutant=None):
    """float64 evaluation of the probe over ALL rows of X (float32 values) with the weights W (float32, as read back).  -> dict(out, bound): x_out [T][d],
    or for `head` the logits every row would give as a call's last row [T][V].  mutant: a _Mut - then `out` is the mutated result (tests judge it by the bound of the clean evaluation)."""
    mu = mutant or _Mut(None, 0)
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    T, d = X.shape
    for n in ZERO[probe]:
        assert not np.any(W[n]), f"probe {probe}: {n} must be exactly 0"
    delta = delta_common(d)
    Tj = np.arange(1, T + 1, dtype=np.float64)[:, None]
    g1, g2 = W["g1"].astype(np.float64), W["g2"].astype(np.float64)
    # ---- attention: scores exactly 0, uniform weights
    Lv, Lo = lin_of(W, "wv"), lin_of(W, "wo")
    h, bh = X, np.zeros_like(X)
    if not (Lv.zero or Lo.zero):
        xn1 = mu.norm(_rms_gain(X, g1), X, g1, probe in ("wv", "wo"))
        z = mu.operand(xn1, probe == "wv")
        (V,), (aV,) = Lv.mm([z], [xn1])
        V = mu.product(V, Lv, z, probe == "wv")
        ind_V = (Lv.C + 3) * U * aV
        Vc = V
        if mu.name == "v_late":                                # row r's V lands one cache position late: position r stays 0, position r + 1 holds it
            Vc = V.copy()
            Vc[mu.r + 1], Vc[mu.r] = V[mu.r], 0.0
        A = _cummean(Vc)
        ind_A = _cummean(ind_V) + (Tj + 16) * U * _cummean(np.abs(V))
        z = mu.operand(A, probe == "wo")
        (Y, YV), (aY, bY) = Lo.mm([z, V], [A, ind_A])
        Y = mu.product(Y, Lo, z, probe == "wo")
        h = X + Y
        bh = Lo.C * U * aY + bY + delta * _cummean(np.abs(YV))
    out, bound = h, bh
    # ---- feed-forward
    L1, L3, L2 = lin_of(W, "w1"), lin_of(W, "w3"), lin_of(W, "w2")
    if not L2.zero:
        assert not np.any(bh), "a probe of the FFN needs h = x exactly"
        xn2 = mu.norm(_rms_gain(h, g2), h, g2, probe in ("w13", "w2"))
        z = mu.operand(xn2, probe == "w13")
        (a,), (aa,) = L1.mm([z], [xn2])
        (b,), (ab,) = L3.mm([xn2], [xn2])
        if mutant is not None and probe == "w13":             # a mutant of one w1 row shows through silu'(a) b: it strikes the row (of the first 64) whose b is largest
            mu.m = int(np.argmax(np.abs(b[mu.r, :64])))
        a = mu.product(a, L1, z, probe == "w13")
        ind_a, ind_b = (L1.C + 3) * U * aa, (L3.C + 3) * U * ab
        if mu.name == "pair_swapped":                          # w1 and w3 exchanged for one row pair
            a, b = a.copy(), b.copy()
            a[:, mu.m], b[:, mu.m] = b[:, mu.m].copy(), a[:, mu.m].copy()
        g = _silu(a) * b
        ind_g = np.abs(_dsilu(a) * b) * ind_a + np.abs(_silu(a)) * ind_b + (np.abs(a) + 8) * U * np.abs(g)
        e = _dsilu(a) * a * b + g
        z = mu.operand(g, probe == "w2")
        (Y, Ye), (aY, bY) = L2.mm([z, e], [g, ind_g])
        Y = mu.product(Y, L2, z, probe == "w2")
        out = h + Y
        bound = L2.C * U * aY + bY + delta * np.abs(Ye)
    if mu.name == "residual_missing":
        out = out.copy()
        out[mu.r, mu.c] -= X[mu.r, mu.c]
    if mu.name == "residual_twice":
        out = out.copy()
        out[mu.r, mu.c] += X[mu.r, mu.c]
    if probe != "head":
        return dict(out=out, bound=bound + 2 * U * np.abs(out))
    # ---- final norm and lm_head, for every row as if it were the last of its call
    assert not np.any(bound), "the head probe needs x_out = x exactly"
    Lh = lin_of(W, "output")
    nw = W["norm"].astype(np.float64)
    xn = mu.norm(_rms_gain(out, nw), out, nw, True)
    z = mu.operand(xn, True)
    (lg,), (al,) = Lh.mm([z], [xn])
    clean = lg
    lg = mu.product(lg, Lh, z, True)
    return dict(out=lg, bound=(Lh.C + 3) * U * al + delta * np.abs(clean) + 2 * U * np.abs(clean))


def make_mutant(name, T):
    return _Mut(name, r=min(5, T - 2))


# ------------------------------------------------------------------------------------------------------------------------------------------
# float32 evaluations
# ------------------------------------------------------------------------------------------------------------------------------------------
def _matmul_f32(z, w, blocked, Q):
    """z [n][K] x w [M][K] in float32.  Textbook: one BLAS call.  blocked: 32-wide K blocks summed one after the other; with Q = (q, d) the
    scale-factored int8 form sum_b d_b (sum_k q_k z_k)."""
    f = np.float32
    z = np.ascontiguousarray(z, dtype=f)
    if not blocked:
        return z @ np.ascontiguousarray(w, dtype=f).T
    n, K = z.shape
    src = Q[0].astype(f) if Q is not None else np.asarray(w, dtype=f)
    M = src.shape[0]
    pad = (-K) % 32
    if pad:
        z, src = np.pad(z, ((0, 0), (0, pad))), np.pad(src, ((0, 0), (0, pad)))
    B = (K + pad) // 32
    zb = z.reshape(n, B, 32).transpose(1, 0, 2)                    # [B][n][32]
    wb = src.reshape(M, B, 32).transpose(1, 2, 0)                  # [B][32][M]
    acc = np.zeros((n, M), dtype=f)
    for b in range(B):
        part = zb[b] @ wb[b]
        acc += part * Q[1][None, :, b] if Q is not None else part
    return acc


def f32_eval(probe, W, X, blocked=False, Q=None):
    """The probe in plain float32 numpy over all rows of X.  blocked = False: the textbook order.  blocked = True: every product in 32-wide K blocks,
    and - with Q = {name: (q, d)} - the block-int8 matrices in the scale-factored form."""
    f = np.float32
    X = np.asarray(X, dtype=f)
    T, d = X.shape
    Q = Q or {}
    mm = lambda z, n: _matmul_f32(z, W[n], blocked, Q.get(n))     # noqa: E731

    def rms(x, g):
        ms = np.mean(x * x, axis=1, dtype=f)
        return x * (f(1) / np.sqrt(ms + f(RMS_EPS)))[:, None] * W[g].astype(f)[None, :]

    def silu(a):
        return a / (f(1) + np.exp(-a))

    cnt = np.arange(1, T + 1, dtype=f)[:, None]
    h = X
    if np.any(W["wv"]) and np.any(W["wo"]):
        V = mm(rms(X, "g1"), "wv")
        A = np.cumsum(V, axis=0, dtype=f) / cnt
        h = X + mm(A, "wo")
    out = h
    if np.any(W["w2"]):
        xn2 = rms(h, "g2")
        g = silu(mm(xn2, "w1")) * mm(xn2, "w3")
        out = h + mm(g, "w2")
    if probe == "head":
        out = mm(rms(out, "norm"), "output")
    return out.astype(np.float64)


def ratio(y, ref):
    """The largest |y - ref| / bound (inf when y is not finite); an element off by anything under a bound of 0 counts as inf."""
    err = np.abs(np.asarray(y, dtype=np.float64) - ref["out"])
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / ref["bound"]).max())


def poisoned(obj, on=True):
    """Test instrumentation in front of a call of model A's context or batch (on = False: the twin, returned untouched): the context-owned weight images - ONE
    layer's matrices and the output matrix, which every layer passes through - filled with 0xFF bytes, NaN as fp32 and quant -1 as int8.  A launch that reads a slot
    this call did not fill itself then computes from poison instead of from what the call before left there (with one layer: always the right matrix).  The fill
    must report bytes wherever images exist - a batch of an f16 / block-int4 model from its creation, a context from its second call (its plans are made lazily by
    the first) - and none on an fp32 / block-int8 model.  -> obj"""
    if not on:
        return obj
    n = obj.PoisonWeightImages()
    calls = getattr(obj, "_poisoned_calls", 0)
    obj._poisoned_calls = calls + 1
    if obj.model.weight_type not in (1, 2):
        assert n == 0, f"{n} bytes of weight images on a context of an fp32 / block-int8 model"
    elif hasattr(obj, "pods") or calls >= 1:
        assert n > 0, "no weight image was filled on a context of an f16 / block-int4 model that has plans"
    return obj
