"""numpy restatement of the block-int4 rule (csrc/kernels_q4.h; dtype 2 = ml.TYPE_Q4_0): quantiser, 20-byte blocks, pack and unpack, expansion.

A block is 32 consecutive weights of a row: {float32 d; uint8 qs[16]}, w = d * (n - 8), element 2j in the low nibble of qs[j], element 2j + 1 in the
high one.  The quantiser: d = fl32(max|w| / 7), q = clamp(rint(fl32(w / d)), -7, 7), n = q + 8; d = 0 -> q = 0; a block that holds a NaN or an infinity:
d = NaN, q = 0.  It never emits n = 0."""
import numpy as np

QK = 32
BLOCK_BYTES = 20


def unpack(qs):
    """uint8 [..., 16] -> nibbles n in 0..15, uint8 [..., 32]"""
    qs = np.asarray(qs, np.uint8)
    out = np.empty(qs.shape[:-1] + (32,), np.uint8)
    out[..., 0::2] = qs & 15
    out[..., 1::2] = qs >> 4
    return out


def pack(n):
    """nibbles uint8 [..., 32] (0..15) -> uint8 [..., 16]"""
    n = np.asarray(n, np.uint8)
    assert (n < 16).all()
    return (n[..., 0::2] | (n[..., 1::2] << 4)).astype(np.uint8)


def quantize(w):
    """float32 [rows, K] (K % 32 == 0) -> (d float32 [rows, K/32], n uint8 [rows, K/32, 32])"""
    w = np.ascontiguousarray(w, np.float32)
    rows, K = w.shape
    assert K % QK == 0
    b = w.reshape(rows, K // QK, QK)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        finite = np.isfinite(b).all(axis=2)
        m = np.where(finite, np.abs(np.where(np.isfinite(b), b, 0)).max(axis=2), 0).astype(np.float32)
        d = (m / np.float32(7.0)).astype(np.float32)
        t = np.rint((b / np.where(d > 0, d, np.float32(1))[..., None]).astype(np.float32))   # rint: ties to even, as rintf in the default mode
        q = np.where((d > 0)[..., None], np.clip(t, -7, 7), 0).astype(np.int32)
    d = np.where(finite, d, np.float32(np.nan)).astype(np.float32)
    q = np.where(finite[..., None], q, 0)
    return d, (q + 8).astype(np.uint8)


def expand(d, n):
    """the block-int8 weights with the same quants and scales: (int8 q [rows, K/32, 32], d)"""
    return (n.astype(np.int16) - 8).astype(np.int8), d


def dequantize(d, n):
    """fl32(d * q), float32 [rows, K]"""
    q, d = expand(d, n)
    with np.errstate(invalid="ignore"):
        w = (d[..., None] * q.astype(np.float32)).astype(np.float32)
    return w.reshape(w.shape[0], -1)


def to_blocks(d, n):
    """the interchange / registration bytes: uint8 [rows * K/32 * 20]"""
    rows, nb = d.shape
    out = np.empty((rows, nb, BLOCK_BYTES), np.uint8)
    out[..., :4] = np.ascontiguousarray(d, np.float32).view(np.uint8).reshape(rows, nb, 4)
    out[..., 4:] = pack(n)
    return out.reshape(-1)


def from_blocks(raw, rows, K):
    raw = np.asarray(raw, np.uint8).reshape(rows, K // QK, BLOCK_BYTES)
    d = np.ascontiguousarray(raw[..., :4]).view(np.float32).reshape(rows, K // QK)
    return d, unpack(raw[..., 4:])


def special_blocks():
    """float32 [4, 32]: an all-zero block, a block with one NaN, one with +inf, one with -inf"""
    rng = np.random.default_rng(2)
    b = (rng.standard_normal((4, 32)) * 0.1).astype(np.float32)
    b[0] = 0
    b[1, 5] = np.nan
    b[2, 31] = np.inf
    b[3, 0] = -np.inf
    return b


def tie_blocks():
    """float32 [6, 32]: blocks whose largest magnitude is 7 (d = 1 exactly), so that w / d = w: every tie k + 0.5, k = -7..6, its two neighbours in
    fp32, values next to +-7 and +-0.5, and -0"""
    f = np.float32
    vals = []
    for k in range(-7, 7):
        t = f(k + 0.5)
        vals += [t, np.nextafter(t, f(-10)), np.nextafter(t, f(10))]
    vals += [f(-0.0), f(6.9999995), f(-6.9999995), f(0.49999997), f(-0.49999997)]
    vals = np.array(vals, np.float32)
    per = 31
    nblk = (len(vals) + per - 1) // per
    out = np.zeros((nblk, 32), np.float32)
    for i in range(nblk):
        chunk = vals[i * per:(i + 1) * per]
        out[i, 0] = 7.0 if i % 2 == 0 else -7.0
        out[i, 1:1 + len(chunk)] = chunk
    # the same with d = 2^-3 (an exact power of two: w / d stays exact), and a scale that is not a power of two
    return np.concatenate([out, out * f(0.125), out * f(0.3)]).astype(np.float32)
