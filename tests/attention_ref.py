"""The probe layer's reference (numpy float64), its error bound, two float32 evaluations, and the case matrix of
tests/test_gpu_attention_bound.py and tests/test_attention_bound_cpu.py.  Written from the mathematics of one LLaMA layer; it shares no code with
oracle/oracle.c or with the kernels.

THE PROBE LAYER.  One layer with attention_norm = ffn_norm = 1, wq = a I, wk = b I, wv = wo = I, w1 = w2 = w3 = 0 computes

    xn_t = x_t / sqrt(mean_c x_tc^2 + 1e-5)          RMSNorm over the whole row (all heads)
    q_t = RoPE_t(a xn_t),  k_t = RoPE_t(b xn_t),  v_t = xn_t          RoPE: pair (2i, 2i+1) of every head turned by t * 10000^(-2i/hd)
    s_jt = q_j . k_t / sqrt(hd)  (per head, t <= j),   p_j = softmax_t(s_j),   attn_j = sum_t p_jt v_t
    x_out_j = x_j + wo attn_j + w2 (...) = x_j + attn_j

I x and 0 x are exact in every summation order, so x_out shows every row of the attention kernel's output behind one rounding of the add.  The
reference takes the weights as they are READ BACK from the device (block-int8 models: the dequantised diagonals, which are no longer exactly a, b, 1),
multiplies with them in full (any matrix works), and requires w2 == 0.

THE SEQUENCE.  A case is one sequence X[T][d] (row t sits at position t) fed to a context in calls (n rows at `past`); the keys of row j are rows 0..j.
Every head carries its scores in its two lowest-frequency RoPE pairs (channels hd-4..hd-1), written PRE-ROTATED (angle phi - t * theta), so that behind
RoPE row t holds amplitude * (cos phi_t, sin phi_t) whatever its position: s_jt = G * (A_j A_t cos(phi_j - phi_t) + A2_j A2_t cos(phi2_j - phi2_t)) with
G = a b H sqrt(hd) when the amplitudes of a row are normalised to sum A^2 = 1 over its heads.  q and k are the same vector up to the gains, so a key can
only beat the query's own key through a NEGATIVE gain product (winner = the key pointing away from the query) or through a larger amplitude (paid for by the
other heads of the row: RMSNorm fixes the row's energy).  The remaining channels carry small random values (2^-12 of the row): the V content every output
column mixes, too small to move a score by more than 1e-4.

THE BOUND (u = 2^-24), for query j, head h, output column c, T_j = j + 1 visible keys:

    eps_j   = (hd + 8) u max_t scale sum_c |q_jc| |k_tc|
    |attn - ref| <= B_jc = (expm1(2 eps_j) + (T_j + 16) u) sum_t p_jt |v_tc|
    |x_out - ref| <= (|wo| B_j)_c + 2 u |x_out_jc|

counted as follows.  A float32 dot product of hd terms, in any order, with or without FMA, errs by at most hd u sum|q_c k_c| (first order); q and k themselves
carry the roundings of the norm (sum of squares, rsqrt, two multiplies), of the gain and of RoPE (two products and an add per element) and the score one
more for the scale: at most 8 further u relative to sum|q||k|.  A score error of at most eps in every key changes every un-normalised weight by a factor
within exp(+-eps) and the normaliser by the same, so p_t moves by a factor within exp(+-2 eps): the first term.  exp, the sum of T_j weights, the division,
the T_j-term PV sum (first-order bound T_j u sum p|v| for any order), the extra products of a rescaled online softmax and of a merge (at most 3 per tile /
chunk / part level, three levels) and v's own roundings (5) fit in (T_j + 16) u.  The last term is the residual add and the rounding of wo attn.  Ties need
no exception: equal scores are perturbed like any others, and the bound moves the weight between the tied keys by the same factor.

THE COMPARATIVE CHECK.  The worst-case bound is loose (a float32 evaluation stays below 11 % of it, below 1 % on most cases), so a second check compares the error of a
whole call, in units of the rounding floor u sum_t p_t |v_tc| pushed through |wo|,

    E(y) = max over rows and columns of |y - ref| / floor        (at least 1)

between the kernel and a plain float32 numpy evaluation in the reference's order (normalise, then PV, keys in order): E(hip) <= K_SPREAD * E(float32).
K_SPREAD is twice the largest ratio E(A) / E(B) either way between two float32 orders - that textbook order and an online softmax over 32-key tiles, both
behind the same float32 projection - over every case of the matrix with ideal weights, rounded up to a power of two.  Measured by
tests/test_attention_bound_cpu.py::test_spread_of_two_float32_orders (which fails when the measurement no longer gives this constant): largest ratio
MEASURED_SPREAD below (dec-hd32-T63-tie: 61.3 against 3.7 floors; the next are dec-hd128-T127-tie, 152 against 24, and the other single-row tie cases).
It was never fitted to a kernel.  The spread is that wide because a row with a few keys at |score| = 120 turns ONE rounding of a score (120 u) into tens of
floors of output error or into none, whichever way the roundings of the tied keys fall; on every other regime the two orders agree within a factor of 4.
"""
import ctypes as C
import os
import subprocess

import numpy as np

U = 2.0 ** -24
RMS_EPS = 1e-5
K_SPREAD = 64          # 2 * MEASURED_SPREAD rounded up to a power of two
MEASURED_SPREAD = 16.5 # largest E(textbook) / E(tiled) or E(tiled) / E(textbook) over the matrix (test_spread_of_two_float32_orders prints it)
V_NOISE = 2.0 ** -12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# the layer
# ------------------------------------------------------------------------------------------------------------------------------------------
def ideal_weights(d, a, b):
    """The probe layer's weights as set on a float32 model (float64 arrays of float32 values)."""
    eye = np.eye(d)
    return dict(attn_norm=np.ones(d), wq=float(np.float32(a)) * eye, wk=float(np.float32(b)) * eye, wv=eye.copy(), wo=eye.copy())


def _rope(x, pos, hd, dtype):
    """x [T][H][hd]; pair (2i, 2i+1) of every head turned by pos * 10000^(-2i/hd).  The angles and their cos / sin are float64 (then cast)."""
    theta = 10000.0 ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.asarray(pos, dtype=np.float64)[:, None] * theta[None, :]
    c, s = np.cos(ang).astype(dtype)[:, None, :], np.sin(ang).astype(dtype)[:, None, :]
    out = np.empty_like(x)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    out[..., 0::2] = x0 * c - x1 * s
    out[..., 1::2] = x0 * s + x1 * c
    return out


def _project(x, W, H, dtype):
    """-> q, k (roped), v, each [T][H][hd] in dtype."""
    T, d = x.shape
    hd = d // H
    x = x.astype(dtype)
    ms = np.mean(x * x, axis=1, dtype=dtype)
    xn = x * (dtype(1) / np.sqrt(ms + dtype(RMS_EPS)))[:, None] * W["attn_norm"].astype(dtype)[None, :]
    pos = np.arange(T)
    q = _rope((xn @ W["wq"].astype(dtype).T).reshape(T, H, hd), pos, hd, dtype)
    k = _rope((xn @ W["wk"].astype(dtype).T).reshape(T, H, hd), pos, hd, dtype)
    v = (xn @ W["wv"].astype(dtype).T).reshape(T, H, hd)
    return q, k, v


def reference(X, W, H, rows):
    """float64 evaluation of x_out for the query rows `rows` of the sequence X [T][d] (float32 values), with the bound, the floor and per (row, head)
    statistics of the score rows the regime assertions use (masked keys included where the sequence has them)."""
    X = np.asarray(X, dtype=np.float32)
    T, d = X.shape
    hd = d // H
    rows = np.asarray(rows, dtype=np.int64)
    q, k, v = _project(X, W, H, np.float64)
    scale = 1.0 / np.sqrt(hd)
    nq = len(rows)
    attn = np.zeros((nq, H, hd))
    battn = np.zeros((nq, H, hd))
    fattn = np.zeros((nq, H, hd))
    st = {n: np.zeros((nq, H)) for n in ("p1", "p2", "s1", "s2", "s3", "next_masked", "smin")}
    st.update({n: np.zeros((nq, H), dtype=np.int64) for n in ("i1", "i2")})
    st.update({n: np.zeros((nq, H), dtype=bool) for n in ("asc", "desc")})
    tk = np.arange(T)
    for r0 in range(0, nq, 256):
        rr = rows[r0:r0 + 256]
        vis = tk[None, :] <= rr[:, None]
        Tj = (rr + 1).astype(np.float64)
        for h in range(H):
            S = scale * (q[rr, h] @ k[:, h].T)
            Sm = np.where(vis, S, -np.inf)
            m = Sm.max(axis=1)
            e = np.exp(Sm - m[:, None])
            p = e / e.sum(axis=1)[:, None]
            attn[r0:r0 + 256, h] = p @ v[:, h]
            A = np.where(vis, scale * (np.abs(q[rr, h]) @ np.abs(k[:, h]).T), 0.0).max(axis=1)
            eps = (hd + 8) * U * A
            pv = p @ np.abs(v[:, h])
            battn[r0:r0 + 256, h] = (np.expm1(2 * eps) + (Tj + 16) * U)[:, None] * pv
            fattn[r0:r0 + 256, h] = U * pv
            # statistics
            order = np.argsort(-Sm, axis=1, kind="stable")[:, :3]
            ar = np.arange(len(rr))
            sl = slice(r0, r0 + 256)
            st["i1"][sl, h], st["p1"][sl, h], st["s1"][sl, h] = order[:, 0], p[ar, order[:, 0]], Sm[ar, order[:, 0]]
            if T > 1:
                st["i2"][sl, h], st["p2"][sl, h], st["s2"][sl, h] = order[:, 1], p[ar, order[:, 1]], Sm[ar, order[:, 1]]
            st["s3"][sl, h] = Sm[ar, order[:, 2]] if T > 2 else -np.inf
            st["smin"][sl, h] = np.where(vis, S, np.inf).min(axis=1)
            nxt = np.minimum(rr + 1, T - 1)
            st["next_masked"][sl, h] = np.where(rr + 1 < T, S[ar, nxt], np.nan)
            # monotone over the visible keys and the first masked one
            dS = np.diff(S, axis=1)
            upto = tk[None, :-1] <= rr[:, None]          # difference t -> t+1 counts for t <= j (t + 1 = j + 1 is the first masked key)
            st["asc"][sl, h] = np.all(np.where(upto, dS > 0, True), axis=1)
            st["desc"][sl, h] = np.all(np.where(upto, dS < 0, True), axis=1)
    wo = W["wo"]
    out = X[rows].astype(np.float64) + attn.reshape(nq, d) @ wo.T
    bound = battn.reshape(nq, d) @ np.abs(wo).T + 2 * U * np.abs(out)
    floor = fattn.reshape(nq, d) @ np.abs(wo).T
    return dict(out=out, bound=bound, floor=floor, stats=st)


# ------------------------------------------------------------------------------------------------------------------------------------------
# float32 evaluations
# ------------------------------------------------------------------------------------------------------------------------------------------
def f32_textbook(X, W, H, rows):
    """float32, the reference's order: scores, max, exp, normalise, then PV with the keys in order."""
    f = np.float32
    X = np.asarray(X, dtype=f)
    T, d = X.shape
    hd = d // H
    rows = np.asarray(rows, dtype=np.int64)
    q, k, v = _project(X, W, H, f)
    scale = f(1.0 / np.sqrt(hd))
    nq = len(rows)
    Tmax = int(rows.max()) + 1
    P = np.zeros((H, nq, Tmax), dtype=f)
    vis = np.arange(Tmax)[None, :] <= rows[:, None]
    for h in range(H):
        S = np.where(vis, (q[rows, h] @ k[:Tmax, h].T) * scale, f(-np.inf)).astype(f)
        e = np.exp(S - S.max(axis=1)[:, None]).astype(f)
        P[h] = e / e.sum(axis=1, dtype=f)[:, None]
    acc = np.zeros((H, nq, hd), dtype=f)
    for t in range(Tmax):
        acc += P[:, :, t, None] * v[t][:, None, :]
    attn = acc.transpose(1, 0, 2).reshape(nq, d)
    return (X[rows] + attn @ W["wo"].astype(f).T).astype(np.float64)


MISTAKES = ("mask_wide", "diag_dropped", "tile_last_dropped", "chunk_last_dropped", "rescale_skipped", "merge_crossed", "part_sum_unscaled", "head_v_shifted",
            "stale_included")


def f32_tiled(X, W, H, rows, call_end=None, groups="single", mistake=None):
    """float32 online softmax over 32-key tiles, as a tiled kernel works: per key group a running (max, sum, accumulator) rescaled when the maximum rises,
    the groups merged at the end (M = max m_g, w_g = exp(m_g - M), out = sum acc_g w_g / sum l_g w_g).  groups: "single", "pair" (even / odd tiles: the two
    wave pairs of a flash block), "chunk" (128 keys: split decode and, for the emulation, a flash part).  mistake: one of MISTAKES, or None for the clean
    evaluation.  call_end: the first position behind the call (its cache row is stale: NaN here when the sequence has no such row)."""
    f = np.float32
    X = np.asarray(X, dtype=f)
    T, d = X.shape
    hd = d // H
    rows = np.asarray(rows, dtype=np.int64)
    assert mistake is None or mistake in MISTAKES
    q, k, v = _project(X, W, H, f)
    nan_row = np.full((1, H, hd), np.nan, dtype=f)
    k, v = np.concatenate([k, nan_row]), np.concatenate([v, nan_row])     # index T: a stale cache row no call of the sequence wrote
    scale = f(1.0 / np.sqrt(hd))
    nq = len(rows)
    limit = rows + 1                                  # keys [0, limit) are visible
    if mistake == "mask_wide":
        limit = limit + 1
    Tmax = int(limit.max())
    ntiles = (Tmax + 31) // 32
    gid = {"single": lambda t: 0, "pair": lambda t: t & 1, "chunk": lambda t: t // 4}[groups]
    G = max(gid(t) for t in range(ntiles)) + 1
    attn = np.zeros((nq, H, hd), dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(H):
            hv = (h + 1) % H if mistake == "head_v_shifted" else h
            m = np.full((G, nq), -np.inf, dtype=f)
            l = np.zeros((G, nq), dtype=f)
            acc = np.zeros((G, nq, hd), dtype=f)
            for ti in range(ntiles):
                t0, t1 = ti * 32, min(ti * 32 + 32, T + 1)
                tt = np.arange(t0, t1)
                vis = tt[None, :] < limit[:, None]
                if mistake == "diag_dropped":
                    vis &= tt[None, :] != rows[:, None]
                if mistake == "tile_last_dropped":
                    vis &= ~((tt[None, :] % 32 == 31) & (tt[None, :] < rows[:, None]))
                if mistake == "chunk_last_dropped":
                    vis &= ~((tt[None, :] % 128 == 127) & (tt[None, :] < rows[:, None]))
                if mistake == "stale_included" and call_end is not None:
                    vis |= np.broadcast_to(tt[None, :] == min(call_end, T), vis.shape)
                if not vis.any():
                    continue
                g = gid(ti)
                s = ((q[rows, h] @ k[t0:t1, h].T) * scale).astype(f)
                s = np.where(vis, s, f(-np.inf))
                m_new = np.maximum(m[g], s.max(axis=1))
                dead = np.isneginf(m_new)                                          # nothing visible for this row so far
                alpha = np.where(np.isneginf(m[g]), f(0), np.exp(m[g] - np.where(dead, f(0), m_new))).astype(f)
                e = np.where(vis, np.exp(s - np.where(dead, f(0), m_new)[:, None]), f(0)).astype(f)
                if mistake == "rescale_skipped":
                    alpha = np.where(np.isneginf(m[g]), f(0), f(1))
                vt = np.where(vis.any(axis=0)[:, None], v[t0:t1, hv], f(0))         # (rows nobody sees are not loaded: 0 * NaN would spoil the product)
                l[g] = l[g] * alpha + e.sum(axis=1, dtype=f)
                acc[g] = acc[g] * alpha[:, None] + e @ vt
                m[g] = m_new
            M = m.max(axis=0)
            w = np.where(np.isneginf(m), f(0), np.exp(m - M[None, :])).astype(f)
            wl = w
            if mistake == "merge_crossed" and G == 2:
                w = wl = w[::-1]
            if mistake == "part_sum_unscaled":
                wl = np.where(np.isneginf(m), f(0), f(1))
            L = (l * wl).sum(axis=0, dtype=f)
            attn[:, h] = (acc * w[:, :, None]).sum(axis=0, dtype=f) / L[:, None]
    return (X[rows] + attn.reshape(nq, d) @ W["wo"].astype(f).T).astype(np.float64)


def through_final_norm(ref, W):
    """The reference of a WHOLE one-layer probe model (norm = 1, output = I, vocab = d): logits = output (x_out / sqrt(mean x_out^2 + 1e-5) * norm).  With
    y = x_out / r: |dy_c| <= B_c / r + |y_c| sum_k |x_out_k| B_k / (d r^2) (first order in the bound B of x_out), plus (d + 8) u |y_c| for the float32 sum
    of d squares, the square root, the division, the product with norm and the rounding of output y."""
    out, d = ref["out"], ref["out"].shape[1]
    r = np.sqrt((out * out).mean(axis=1) + RMS_EPS)[:, None]
    y = out / r * W["norm"][None, :]
    by = ref["bound"] / r + np.abs(y) * (np.abs(out) * ref["bound"]).sum(axis=1)[:, None] / (d * r * r) + (d + 8) * U * np.abs(y)
    A = np.abs(W["output"])
    # the floor of the comparative check: the attention's floor through the norm, plus the one rounding u |y| no float32 logit can avoid (without it a
    # column the attention adds nothing to - floor 0 - would be judged by the norm's roundings alone)
    return dict(out=y @ W["output"].T, bound=by @ A.T, floor=(ref["floor"] / r + U * np.abs(y)) @ A.T, stats=ref["stats"])


def f32_final_norm(x_out, W):
    f = np.float32
    x = np.asarray(x_out, dtype=f)
    r = np.sqrt(np.mean(x * x, axis=1, dtype=f) + f(RMS_EPS))
    return ((x / r[:, None] * W["norm"].astype(f)[None, :]) @ W["output"].astype(f).T).astype(np.float64)


def decoy_rows(T, H, hd, seed=99):
    """Rows for a stale cache: every key points away from an ordinary query (it wins under a negative gain product) and carries values two hundred
    times the usual ones."""
    X = build_sequence(T, H, hd, [spec_keys(T, range(T)) for _ in range(H)], seed).reshape(T, H, hd)
    X[:, :, :hd - 4] *= np.float32(200.0)
    return X.reshape(T, H * hd)


def case_error(y, ref):
    """E(y): the largest error of a call in units of the rounding floor (at least 1); inf when y is not finite."""
    err = np.abs(np.asarray(y, dtype=np.float64) - ref["out"])
    if not np.all(np.isfinite(err)):
        return float("inf")
    return max(1.0, float((err / np.maximum(ref["floor"], np.finfo(np.float64).tiny)).max()))


def bound_ratio(y, ref):
    """The largest |y - ref| / bound of a call (inf when y is not finite): <= 1 passes."""
    err = np.abs(np.asarray(y, dtype=np.float64) - ref["out"])
    if not np.all(np.isfinite(err)):
        return float("inf")
    return float(np.where(err == 0, 0.0, err / np.maximum(ref["bound"], np.finfo(np.float64).tiny)).max())


# ------------------------------------------------------------------------------------------------------------------------------------------
# regimes: per head (A, phi, A2, phi2), each an array over the rows of the sequence
# ------------------------------------------------------------------------------------------------------------------------------------------
def build_sequence(T, H, hd, heads, seed):
    """X [T][d] float32 from per-head specs (A, phi, A2, phi2: scalars or [T] arrays; amplitudes relative, every row normalised to sum A^2 + A2^2 = 1)."""
    rng = np.random.default_rng(seed)
    d = H * hd
    pos = np.arange(T, dtype=np.float64)
    X = np.zeros((T, H, hd))
    A = np.array([[np.broadcast_to(np.asarray(s[i], dtype=np.float64), (T,)) for i in (0, 2)] for s in heads])   # [H][2][T]
    A = A / np.sqrt((A ** 2).sum(axis=(0, 1)))[None, None, :]
    for h, s in enumerate(heads):
        for pi, (amp, phi) in enumerate(((A[h, 0], s[1]), (A[h, 1], s[3]))):
            i = hd // 2 - 1 - pi                                             # pair index: the lowest frequency, then the next
            theta = 10000.0 ** (-(2.0 * i) / hd)
            ang = np.broadcast_to(np.asarray(phi, dtype=np.float64), (T,)) - pos * theta
            X[:, h, 2 * i] = amp * np.cos(ang)
            X[:, h, 2 * i + 1] = amp * np.sin(ang)
        X[:, h, :hd - 4] = V_NOISE * rng.standard_normal((T, hd - 4))
    return X.reshape(T, d).astype(np.float32)


def spec_diffuse(T, rng, amp=1.0):
    return (amp, rng.uniform(0, 2 * np.pi, T), amp, rng.uniform(0, 2 * np.pi, T))


def spec_keys(T, keys, amp=1.0):
    """The listed keys point away from every other row (phi = pi against 0): under a negative gain product they win every later query."""
    phi = np.zeros(T)
    phi[list(keys)] = np.pi
    return (amp, phi, 0.0, 0.0)


DIAG_ROWS = 24


def diag_rows(T):
    """The rows of a "diag" sequence that are one-hot on their own key: the last 24 (row 0 keeps the common direction)."""
    return np.arange(max(1, T - DIAG_ROWS), T)


def spec_diag(T, amp=1.0):
    """One-hot on the DIAGONAL under a positive gain product: the last 24 rows point in 24 directions of a 5 x 5 grid over the two pairs (72 degrees apart:
    cos <= 0.31 in at least one pair), every earlier row in the 25th.  A row's own key scores G A^2, every other at most 0.655 of that."""
    phi, phi2 = np.zeros(T), np.zeros(T)
    for k, r in enumerate(diag_rows(T), start=1):
        phi[r], phi2[r] = 2 * np.pi * (k % 5) / 5, 2 * np.pi * (k // 5) / 5
    return (amp, phi, amp, phi2)


def spec_ramp(T, lo=0.2, hi=0.8, amp=1.0):
    """Amplitude^2 rising linearly with the key index (the complementary head falls): scores monotone in the key index, masked keys included."""
    f = lo + (hi - lo) * np.arange(T) / max(T - 1, 1)
    return (amp * np.sqrt(f), 0.0, 0.0, 0.0)


def spec_offset(T, rng, amp=1.0, ripple=0.07):
    """Every key at the same large score through the lowest pair, a diffuse ripple through the next one."""
    return (amp, 0.0, amp * ripple, rng.uniform(0, 2 * np.pi, T))


class Case:
    """One sequence and the calls that feed it to a context.  setup calls build the cache and are not checked (a wrong cache row shows in the checked
    calls behind it); `calls` are checked row by row and name the attention route they must take."""

    def __init__(self, name, route, H, hd, ctx, calls, regime, g, setup=(), keys=(), T=None, lazy=None):
        """lazy: a callable -> (route, keys) evaluated on first use (the cut flash cases ask the work list, which has to be compiled)."""
        self.name, self._route, self.H, self.hd, self.ctx, self.calls, self.setup = name, route, H, hd, ctx, list(calls), list(setup)
        self.regime, self.g, self._keys, self._lazy = regime, g, tuple(keys), lazy
        self.T = T or max(p + n for n, p in self.calls + self.setup)
        self.d = H * hd
        # gains: G = a b H sqrt(hd) = g  (see the module docstring); one-hot / tie / "off-" regimes need a negative product
        mag = np.sqrt(abs(g) / (H * np.sqrt(hd)))
        self.a, self.b = float(np.float32(mag)), float(np.float32(np.copysign(mag, g)))

    def _resolve(self):
        if self._lazy is not None:
            self._route, keys = self._lazy()
            self._keys, self._lazy = tuple(keys), None

    @property
    def route(self):
        self._resolve()
        return self._route

    @property
    def keys(self):
        self._resolve()
        return self._keys

    def heads(self):
        rng = np.random.default_rng(sum(map(ord, self.name)))
        T, H = self.T, self.H
        weak = 0.07     # amplitude of a diffuse head next to a strong one: its scores are G * 0.005 (two pairs)
        if self.regime == "diffuse":
            hs = [spec_diffuse(T, rng) for _ in range(H)]
        elif self.regime in ("onehot", "tie"):         # head 1 carries the keys, the others are diffuse (head 0 first: a head-index slip shows)
            hs = [spec_diffuse(T, rng, weak) for _ in range(H)]
            hs[1] = spec_keys(T, self.keys)
            if H > 2:
                hs[H - 1] = spec_keys(T, self.keys[::-1][:1])     # a second strong head with ONE of the keys
        elif self.regime == "diag":                    # head 1 one-hot on the diagonal in its last rows, the others diffuse
            hs = [spec_diffuse(T, rng, weak) for _ in range(H)]
            hs[1] = spec_diag(T)
        elif self.regime == "ramp":                    # head 0 rises, head 1 falls (g > 0; g < 0 swaps them), further heads diffuse
            up = spec_ramp(T)
            hs = [up, (np.sqrt(1.0 - up[0] ** 2), 0.0, 0.0, 0.0)] + [spec_diffuse(T, rng, weak) for _ in range(H - 2)]
        elif self.regime == "offset":                  # head 0: common offset + ripple; head 1 diffuse
            hs = [spec_offset(T, rng)] + [spec_diffuse(T, rng, weak) for _ in range(H - 1)]
        else:
            raise ValueError(self.regime)
        return hs

    def sequence(self):
        return build_sequence(self.T, self.H, self.hd, self.heads(), seed=sum(map(ord, self.name)) + 1)

    def weights(self):
        return ideal_weights(self.d, self.a, self.b)

    def steps(self):
        """every call in position order: (n, past, checked)"""
        st = sorted([(p, n, True) for n, p in self.calls] + [(p, n, False) for n, p in self.setup])
        pos = 0
        for p, n, _ in st:
            assert p == pos, (self.name, st)          # the calls tile the sequence without gaps
            pos += n
        return [(n, p, chk) for p, n, chk in st]

    def checked_rows(self):
        return np.concatenate([np.arange(p, p + n) for n, p in sorted(self.calls, key=lambda c: c[1])])

    def __repr__(self):
        return self.name


def check_regime(case, ref, rows):
    """Asserts the case's defining property on the float64 reference of the rows of one call; returns the number of (row, head) pairs it held for."""
    st, H = ref["stats"], case.H
    rows = np.asarray(rows)
    held = 0
    if case.regime == "diffuse":
        sel = rows + 1 >= 64
        assert np.all(st["p1"][sel] < 0.2), (case, float(st["p1"][sel].max()))
        held = int(sel.sum()) * H
    elif case.regime == "onehot":
        w = case.keys[0]
        sel = rows > w                                   # later queries: the key wins with a margin > 30 and the output is its V row
        assert np.all(st["i1"][sel, 1] == w) and np.all(st["s1"][sel, 1] - st["s2"][sel, 1] > 30), case
        assert np.all(st["p1"][sel, 1] > 1 - 1e-12), case
        held = int(sel.sum())
        if np.any(rows == w) and w > 0:                  # the key's own row: every earlier key ties, its own is out by the same margin
            i = int(np.nonzero(rows == w)[0][0])
            assert st["s1"][i, 1] - st["smin"][i, 1] > 30 and st["i1"][i, 1] != w, case
        for h in range(H):                               # the diffuse heads stay diffuse
            if h != 1 and not (H > 2 and h == H - 1):
                assert np.all(st["p1"][rows + 1 >= 64, h] < 0.2), case
    elif case.regime == "diag":
        sel = np.isin(rows, diag_rows(case.T))          # every one of these rows: its own key wins with a margin > 30, the output is its own V row
        assert np.all(st["i1"][sel, 1] == rows[sel]) and np.all(st["s1"][sel, 1] - st["s2"][sel, 1] > 30) and np.all(st["p1"][sel, 1] > 1 - 1e-12), case
        held = int(sel.sum())
    elif case.regime == "tie":
        w1, w2 = case.keys
        sel = rows > max(w1, w2)
        top2 = np.sort(np.stack([st["i1"][sel, 1], st["i2"][sel, 1]], axis=1), axis=1)
        assert np.all(top2 == np.array(sorted((w1, w2)))[None, :]), case                      # the two keys share the weight: the output is the mean of their V rows
        assert np.all(np.abs(st["p1"][sel, 1] - 0.5) < 1e-3) and np.all(np.abs(st["p2"][sel, 1] - 0.5) < 1e-3), (case, st["p1"][sel, 1], st["p2"][sel, 1])
        assert np.all(st["s2"][sel, 1] - st["s3"][sel, 1] > 30), case
        held = int(sel.sum())
    elif case.regime == "ramp":
        up, down = (0, 1) if case.g > 0 else (1, 0)
        assert np.all(st["asc"][:, up]) and np.all(st["desc"][:, down]), case
        nm = st["next_masked"]
        has = ~np.isnan(nm[:, up])
        assert np.all(nm[has, up] > st["s1"][has, up]), case          # the first masked key would beat every visible one
        assert np.all(st["i1"][:, down] == 0), case                    # the running maximum never rises: key 0 holds it
        held = 2 * len(rows)
    elif case.regime == "offset":
        lo, hi = (80, 150) if case.g > 0 else (-150, -80)
        assert np.all(st["smin"][:, 0] > lo) and np.all(st["s1"][:, 0] < hi), (case, float(st["smin"][:, 0].min()), float(st["s1"][:, 0].max()))
        assert np.all(st["s1"][:, 0] - st["smin"][:, 0] < 20), case      # a diffuse row on top of the offset
        held = len(rows)
    return held


# ------------------------------------------------------------------------------------------------------------------------------------------
# the work list of the flash kernel (csrc/attn_worklist.h through tests/attn_worklist_shim.cpp)
# ------------------------------------------------------------------------------------------------------------------------------------------
_WL = None


def worklist_lib(tmpdir=None):
    global _WL
    if _WL is None:
        import atexit
        import shutil
        import tempfile
        if tmpdir is None:
            tmpdir = tempfile.mkdtemp(prefix="wl")
            atexit.register(shutil.rmtree, tmpdir, True)
        so = os.path.join(tmpdir, "libwl.so")
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", so,
                        os.path.join(ROOT, "tests", "attn_worklist_shim.cpp")], check=True)
        lib = C.CDLL(so)
        lib.worklist.argtypes = [C.c_uint] * 4 + [C.POINTER(C.c_uint), C.POINTER(C.c_ushort)]
        for fn in (lib.steps, lib.parts, lib.part_begin):
            fn.restype = C.c_uint
            fn.argtypes = [C.c_uint] * 3 if fn is not lib.parts else [C.c_uint] * 2
        _WL = lib
    return _WL


def flash_parts(n, past, H, slots=512):
    """-> (cut, pmax, [first key of every part of the LAST query block but the first part]) for a flash call; slots = 2 * CUs (512 on an MI355X)."""
    lib = worklist_lib()
    out = (C.c_uint * 6)()
    work = (C.c_ushort * 160)()
    lib.worklist(n, past, H, slots, out, work)
    chunk, qb_cut, pmax, nqb = out[0], out[1], out[2], out[5]
    cut = chunk != 0 and qb_cut < nqb
    st = lib.steps(past, n, nqb - 1)
    np_ = lib.parts(st, chunk)
    return cut, int(pmax), [int(lib.part_begin(st, np_, pt)) * 64 for pt in range(1, np_)]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the case matrix
# ------------------------------------------------------------------------------------------------------------------------------------------
G_STRONG = 120.0     # scores of a strong head: +-120 (one-hot margin 240, offset 120)


def _decode(T):
    """a single query behind T - 1 cached keys, the cache built by one prompt"""
    return dict(calls=[(1, T - 1)], setup=[(T - 1, 0)] if T > 1 else [])


def case_matrix(slots=512):
    cs = []
    # ---- k_attention, n = 1, ctx <= 256: every softmax branch (T <= 64, <= 128, longer) and the strided path of the other head dims
    for hd, H in ((128, 2), (64, 2), (32, 4), (256, 2)):
        for T in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256):
            route = f"k_attention/hd{hd}/n1"
            cs.append(Case(f"dec-hd{hd}-T{T}-diffuse", route, H, hd, 256, regime="diffuse", g=1.0, **_decode(T)))
            if T >= 2:
                cs.append(Case(f"dec-hd{hd}-T{T}-ramp", route, H, hd, 256, regime="ramp", g=60.0 if T % 2 else -60.0, **_decode(T)))
            if T >= 3:
                for nm, w in (("first", 0), ("prev", T - 2), ("t63", 63), ("t64", 64), ("t127", 127), ("t128", 128)):
                    if w <= T - 2:
                        cs.append(Case(f"dec-hd{hd}-T{T}-onehot-{nm}", route, H, hd, 256, regime="onehot", keys=(w,), g=-G_STRONG, **_decode(T)))
                cs.append(Case(f"dec-hd{hd}-T{T}-tie", route, H, hd, 256, regime="tie", keys=(0, T - 2), g=-G_STRONG, **_decode(T)))
            if T >= 2:
                cs.append(Case(f"dec-hd{hd}-T{T}-onehot-diag", route, H, hd, 256, regime="diag", g=G_STRONG, **_decode(T)))
            cs.append(Case(f"dec-hd{hd}-T{T}-offset", route, H, hd, 256, regime="offset", g=G_STRONG if T % 2 else -G_STRONG, **_decode(T)))
    # ---- k_attention, prompts of 2, 8, 31 rows at past = 0 and behind a cache
    for n in (2, 8, 31):
        for past in (0, 40):
            T = past + n
            kw = dict(calls=[(n, past)], setup=[(past, 0)] if past else [])
            route = f"k_attention/hd128/n{n}"
            cs.append(Case(f"rows{n}-p{past}-diffuse", route, 2, 128, 256, regime="diffuse", g=1.0, **kw))
            cs.append(Case(f"rows{n}-p{past}-ramp", route, 2, 128, 256, regime="ramp", g=60.0, **kw))
            cs.append(Case(f"rows{n}-p{past}-onehot-first", route, 2, 128, 256, regime="onehot", keys=(0,), g=-G_STRONG, **kw))
            if past:
                cs.append(Case(f"rows{n}-p{past}-onehot-pastm1", route, 2, 128, 256, regime="onehot", keys=(past - 1,), g=-G_STRONG, **kw))
                cs.append(Case(f"rows{n}-p{past}-onehot-past", route, 2, 128, 256, regime="onehot", keys=(past,), g=-G_STRONG, **kw))
                cs.append(Case(f"rows{n}-p{past}-tie", route, 2, 128, 256, regime="tie", keys=(past - 1, past), g=-G_STRONG, **kw))
            cs.append(Case(f"rows{n}-p{past}-onehot-diag", route, 2, 128, 256, regime="diag", g=G_STRONG, **kw))
            cs.append(Case(f"rows{n}-p{past}-offset", route, 2, 128, 256, regime="offset", g=-G_STRONG, **kw))
    # ---- split + combine: consecutive positions in one context, across the chunk counts 1|2, 2|3, 8|9, 16|17 and up to ctx - 1
    for ctx, walks in ((320, (127, 128, 129, 255, 256, 257, 318, 319)), (1152, (1023, 1024, 1025, 1150, 1151)), (2304, (2047, 2048, 2049, 2302, 2303))):
        nch = (ctx + 127) // 128
        route = f"k_attention_split/c{nch}/n1 k_attention_combine/c{nch}/n1"
        kw = dict(calls=[(1, p) for p in range(walks[0], walks[-1] + 1)] if ctx == 320 else [(1, p) for p in walks], setup=[(walks[0], 0)])
        if ctx != 320:     # the positions between the walked ones are filled by setup prompts
            kw = dict(calls=[(1, p) for p in walks], setup=[(walks[0], 0)] + [(b - a - 1, a + 1) for a, b in zip(walks, walks[1:]) if b - a > 1])
        cs.append(Case(f"split{ctx}-diffuse", route, 2, 128, ctx, regime="diffuse", g=1.0, **kw))
        cs.append(Case(f"split{ctx}-ramp", route, 2, 128, ctx, regime="ramp", g=60.0, **kw))
        cs.append(Case(f"split{ctx}-onehot-diag", route, 2, 128, ctx, regime="diag", g=G_STRONG, **kw))
        cs.append(Case(f"split{ctx}-offset", route, 2, 128, ctx, regime="offset", g=-G_STRONG, **kw))
        for nm, w in (("first", 0), ("c0last", 127), ("c1first", 128), ("c7last", 1023), ("c8first", 1024), ("c15last", 2047), ("c16first", 2048)):
            if w < walks[-1]:
                cs.append(Case(f"split{ctx}-onehot-{nm}", route, 2, 128, ctx, regime="onehot", keys=(w,), g=-G_STRONG, **kw))
        cs.append(Case(f"split{ctx}-tie-chunks", route, 2, 128, ctx, regime="tie", keys=(5, walks[0] - 2), g=-G_STRONG, **kw))
        if ctx > 320:      # the two maxima eight chunks apart: in different prefetch batches of the combine
            cs.append(Case(f"split{ctx}-tie-batches", route, 2, 128, ctx, regime="tie", keys=(100, 1022), g=-G_STRONG, **kw))
    # ---- flash, uncut: odd and even tile counts, ragged last blocks with 1, 33 and 63 live queries
    for n, past in ((32, 0), (33, 31), (64, 0), (64, 37), (65, 0), (65, 64), (97, 1), (97, 31), (127, 0), (127, 37), (191, 0), (191, 64)):
        T = past + n
        kw = dict(calls=[(n, past)], setup=[(past, 0)] if past else [])
        route = "k_attn_flash/uncut/p1"
        cs.append(Case(f"flash-n{n}-p{past}-diffuse", route, 2, 128, 256, regime="diffuse", g=1.0, **kw))
        cs.append(Case(f"flash-n{n}-p{past}-ramp", route, 2, 128, 256, regime="ramp", g=60.0 if n % 2 else -60.0, **kw))
        cs.append(Case(f"flash-n{n}-p{past}-onehot-diag", route, 2, 128, 256, regime="diag", g=G_STRONG, **kw))
        cs.append(Case(f"flash-n{n}-p{past}-offset", route, 2, 128, 256, regime="offset", g=G_STRONG if past % 2 else -G_STRONG, **kw))
        for nm, w in (("first", 0), ("t31", 31), ("t32", 32), ("t63", 63), ("t64", 64), ("pastm1", past - 1), ("past", past), ("prev", T - 2)):
            if 0 <= w <= T - 2:
                cs.append(Case(f"flash-n{n}-p{past}-onehot-{nm}", route, 2, 128, 256, regime="onehot", keys=(w,), g=-G_STRONG, **kw))
        if T >= 70:
            cs.append(Case(f"flash-n{n}-p{past}-tie-tiles", route, 2, 128, 256, regime="tie", keys=(31, 32), g=-G_STRONG, **kw))       # neighbouring tiles = the two wave pairs
            cs.append(Case(f"flash-n{n}-p{past}-tie-samepair", route, 2, 128, 256, regime="tie", keys=(3, 66), g=-G_STRONG, **kw))    # tiles 0 and 2: one wave pair
    # ---- flash, cut by key range: winners and ties on the part boundaries the work list itself gives
    for n, past, ctx in ((64, 1920, 2048), (163, 1900, 2304), (700, 0, 768)):
        def at(kind, n=n, past=past):
            """(route, keys) of a cut case, from the work list itself (asked when the case is first used)"""
            def resolve():
                cut, pmax, firsts = flash_parts(n, past, 2, slots)
                assert cut and firsts, (n, past, "the work list no longer cuts this shape: pick one it does")
                b = firsts[len(firsts) // 2]
                keys = {"none": (), "first": (0,), "partlast": (b - 1,), "partfirst": (b,), "tie-parts": (b - 1, b), "tie-farparts": (1, firsts[-1] + 1)}[kind]
                return f"k_attn_flash/cut/p{pmax} k_attn_flash_combine/p{pmax}", keys
            return resolve
        kw = dict(calls=[(n, past)], setup=[(past, 0)] if past else [])
        cs.append(Case(f"cut-n{n}-p{past}-diffuse", None, 2, 128, ctx, regime="diffuse", g=1.0, lazy=at("none"), **kw))
        cs.append(Case(f"cut-n{n}-p{past}-ramp", None, 2, 128, ctx, regime="ramp", g=60.0, lazy=at("none"), **kw))
        cs.append(Case(f"cut-n{n}-p{past}-offset", None, 2, 128, ctx, regime="offset", g=-G_STRONG, lazy=at("none"), **kw))
        cs.append(Case(f"cut-n{n}-p{past}-onehot-diag", None, 2, 128, ctx, regime="diag", g=G_STRONG, lazy=at("none"), **kw))
        for nm in ("first", "partlast", "partfirst"):
            cs.append(Case(f"cut-n{n}-p{past}-onehot-{nm}", None, 2, 128, ctx, regime="onehot", g=-G_STRONG, lazy=at(nm), **kw))
        cs.append(Case(f"cut-n{n}-p{past}-tie-parts", None, 2, 128, ctx, regime="tie", g=-G_STRONG, lazy=at("tie-parts"), **kw))
        cs.append(Case(f"cut-n{n}-p{past}-tie-farparts", None, 2, 128, ctx, regime="tie", g=-G_STRONG, lazy=at("tie-farparts"), **kw))
    # ---- GEMM attention: the other head dims, T not a multiple of 32, behind a cache
    for hd, H in ((32, 4), (64, 2)):
        for n, past in ((32, 0), (56, 0), (70, 0), (130, 0), (70, 21)):
            T = past + n
            kw = dict(calls=[(n, past)], setup=[(past, 0)] if past else [])
            route = f"attention_gemm/hd{hd}/n{n}"
            cs.append(Case(f"gemm-hd{hd}-n{n}-p{past}-diffuse", route, H, hd, 256, regime="diffuse", g=1.0, **kw))
            cs.append(Case(f"gemm-hd{hd}-n{n}-p{past}-ramp", route, H, hd, 256, regime="ramp", g=60.0, **kw))
            cs.append(Case(f"gemm-hd{hd}-n{n}-p{past}-onehot-diag", route, H, hd, 256, regime="diag", g=G_STRONG, **kw))
            cs.append(Case(f"gemm-hd{hd}-n{n}-p{past}-offset", route, H, hd, 256, regime="offset", g=-G_STRONG, **kw))
            for nm, w in (("first", 0), ("t31", 31), ("t32", 32), ("prev", T - 2)):
                if w <= T - 2:
                    cs.append(Case(f"gemm-hd{hd}-n{n}-p{past}-onehot-{nm}", route, H, hd, 256, regime="onehot", keys=(w,), g=-G_STRONG, **kw))
            if T >= 40:
                cs.append(Case(f"gemm-hd{hd}-n{n}-p{past}-tie", route, H, hd, 256, regime="tie", keys=(31, 32), g=-G_STRONG, **kw))
    assert len({c.name for c in cs}) == len(cs)
    return cs
