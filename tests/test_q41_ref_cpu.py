"""tests/q41_ref.py against the Q4_1 rule itself: the error bound, d = 0, the non-finite rule, ggml's byte order."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q41_ref as Q   # noqa: E402


def test_error_bound_on_finite_blocks():
    rng = np.random.default_rng(1)
    w = np.concatenate([(rng.standard_normal((256, 32)) * s + o).astype(np.float32) for s, o in ((1e-3, 0), (0.02, 1), (1.0, -3), (300.0, 7))] + [Q.crafted_blocks()[:5]])
    d, m, n = Q.quantize(w)
    wq = Q.dequantize(d, m, n)
    assert n.max() == 15 and n.min() == 0
    assert np.all(np.abs(w.astype(np.float64) - wq) <= (0.5 + 2.0 ** -18) * d.astype(np.float64))


def test_constant_and_non_finite_blocks():
    w = Q.crafted_blocks()
    d, m, n = Q.quantize(w)
    for k in (0, 5):                                   # d = 0: every nibble 0, the value is m exactly
        assert d[k, 0] == 0 and not n[k].any() and np.array_equal(Q.dequantize(d, m, n)[k], w[k])
    for k in (6, 7, 8):                                # a NaN, an infinity, an overflowing max - min: d = m = NaN, nibbles 0
        assert np.isnan(d[k, 0]) and np.isnan(m[k, 0]) and not n[k].any() and np.isnan(Q.dequantize(d, m, n)[k]).all()


def test_pack_is_ggml_byte_order():
    n = (np.arange(32) * 7 % 16).astype(np.uint8)[None, :]
    raw = Q.to_blocks(np.float32([[0.5]]), np.float32([[-2.0]]), n)
    assert raw.shape == (1, 24)
    assert raw[0, :4].tobytes() == np.float32(0.5).tobytes() and raw[0, 4:8].tobytes() == np.float32(-2.0).tobytes()
    assert all(raw[0, 8 + j] == (int(n[0, 2 * j]) | int(n[0, 2 * j + 1]) << 4) for j in range(16))
    d, m, n2 = Q.from_blocks(raw, 1, 32)
    assert d[0, 0] == 0.5 and m[0, 0] == -2.0 and np.array_equal(n2, n)
