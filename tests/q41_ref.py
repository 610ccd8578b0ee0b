"""numpy restatement of the Q4_1 rule (csrc/kernels_q41.h), written from the rule, not from the kernels.

Block of 32 weights: {float d; float m; uint8 qs[16]} = 24 bytes; element 2j is the low nibble of qs[j], element 2j + 1 the high one; n in [0, 15].
Value:      w' = fl32(d n + m) with ONE rounding (an fma).
Quantiser:  m = min w, d = fl32(fl32(max w - m) / 15), n = clamp(rint(fl32(fl32(w - m) / d)), 0, 15); d = 0 -> n = 0; a block that holds a NaN or an
            infinity, or whose max w - min w is not finite in float32: d = m = NaN, n = 0."""
import numpy as np

F = np.float32


def quantize(w):
    """w float32 [.., K], K % 32 == 0 -> (d [.., K / 32], m [.., K / 32], n uint8 [.., K])"""
    w = np.ascontiguousarray(w, dtype=F)
    b = w.reshape(-1, 32)
    with np.errstate(all="ignore"):
        m = np.min(b, axis=1)
        span = (np.max(b, axis=1) - m).astype(F)
        bad = ~np.all(np.isfinite(b), axis=1) | ~np.isfinite(span)
        d = (span / F(15)).astype(F)
        t = ((b - m[:, None]).astype(F) / np.where(d > 0, d, F(1))[:, None]).astype(F)
        n = np.where((d > 0)[:, None] & ~bad[:, None], np.clip(np.rint(np.where(bad[:, None], F(0), t)), 0, 15), 0).astype(np.uint8)
    d, m = np.where(bad, F(np.nan), d).astype(F), np.where(bad, F(np.nan), m).astype(F)
    blk = w.shape[:-1] + (w.shape[-1] // 32,)
    return d.reshape(blk), m.reshape(blk), n.reshape(w.shape)


def dequantize(d, m, n):
    """w' = fl32(d n + m), one rounding: d n is exact in float64 (24 + 4 bits); the float64 sum is made odd where it is inexact (TwoSum tells), so
    the second rounding, to float32, cannot double-round."""
    p = np.repeat(np.asarray(d, F).astype(np.float64), 32, axis=-1) * np.asarray(n).astype(np.float64)
    a = np.repeat(np.asarray(m, F).astype(np.float64), 32, axis=-1)
    with np.errstate(all="ignore"):
        s = p + a
        z = s - p
        e = (p - (s - z)) + (a - z)                                 # the exact p + a - s
        bits = s.view(np.int64).copy()
        fix = np.isfinite(s) & (e != 0) & ((bits & 1) == 0)
        bits[fix] += np.where((e[fix] > 0) == (s[fix] > 0), 1, -1)   # the odd neighbour on the side of the exact sum
        return bits.view(np.float64).astype(F)


def to_blocks(d, m, n):
    """-> uint8 [blocks][24], the interchange bytes"""
    n = np.asarray(n, np.uint8).reshape(-1, 16, 2)
    out = np.empty((n.shape[0], 24), np.uint8)
    out[:, 0:4] = np.asarray(d, F).reshape(-1, 1).view(np.uint8)
    out[:, 4:8] = np.asarray(m, F).reshape(-1, 1).view(np.uint8)
    out[:, 8:] = n[:, :, 0] | (n[:, :, 1] << 4)
    return out


def from_blocks(raw, rows, K):
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1, 24)
    d, m = raw[:, 0:4].copy().view(F).reshape(rows, K // 32), raw[:, 4:8].copy().view(F).reshape(rows, K // 32)
    n = np.stack([raw[:, 8:] & 15, raw[:, 8:] >> 4], axis=2).reshape(rows, K)
    return d, m, n


def crafted_blocks():
    """float32 [9][32]: constant, all negative, all positive, spanning zero, one outlier, d = 0 at zero, one NaN, one infinity, a finite span that overflows"""
    r = np.random.default_rng(3).standard_normal((9, 32)).astype(F)
    r[0] = F(0.3)
    r[1] = -np.abs(r[1]) - F(0.5)
    r[2] = np.abs(r[2]) + F(0.5)
    r[4] *= F(1e-3); r[4, 17] = F(40.0)
    r[5] = F(0)
    r[6, 5] = np.nan
    r[7, 31] = -np.inf
    r[8, 0], r[8, 1] = F(3e38), F(-3e38)
    return r
