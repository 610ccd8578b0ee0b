"""not-gpu: the numpy restatement of the block-int4 rule (tests/q4_ref.py) against itself: pack / unpack, the expansion to block-int8, the quantiser's
error bound and its rule for zero and non-finite blocks.  tests/test_gpu_q4.py holds the device kernels to this file bit for bit."""
import numpy as np

import q4_ref as Q


def test_pack_and_unpack_are_inverse_over_all_byte_values():
    qs = np.arange(256, dtype=np.uint8).reshape(16, 16)
    n = Q.unpack(qs)
    assert n.shape == (16, 32) and n.max() == 15
    assert (Q.pack(n) == qs).all()
    assert n[0, 0] == 0 and n[0, 1] == 0 and n[1, 2] == 1 and n[1, 3] == 1       # byte 0x11 at index 17: low nibble first
    b = np.array([0xA3], np.uint8).repeat(16)[None]
    assert (Q.unpack(b)[0, 0::2] == 3).all() and (Q.unpack(b)[0, 1::2] == 10).all()
    all_n = np.arange(16, dtype=np.uint8).repeat(2)[None]                        # every nibble value, n = 0 included
    assert (Q.unpack(Q.pack(all_n)) == all_n).all()


def test_expansion_holds_the_same_values():
    rng = np.random.default_rng(0)
    n = rng.integers(0, 16, (8, 4, 32)).astype(np.uint8)
    d = (rng.standard_normal((8, 4)) * 0.01).astype(np.float32)
    q, d8 = Q.expand(d, n)
    assert q.dtype == np.int8 and q.min() == -8 and q.max() == 7 and d8 is d
    w8 = (d8[..., None] * q.astype(np.float32)).astype(np.float32).reshape(8, -1)   # the block-int8 rule: fl32(d * q)
    assert w8.tobytes() == Q.dequantize(d, n).tobytes()
    raw = Q.to_blocks(d, n)
    assert raw.size == 8 * 4 * 20
    d2, n2 = Q.from_blocks(raw, 8, 128)
    assert d2.tobytes() == d.tobytes() and (n2 == n).all()


def test_error_bound_and_quant_range_on_normal_blocks():
    rng = np.random.default_rng(1)
    w = np.concatenate([(rng.standard_normal((512, 32)) * s).astype(np.float32) for s in (1e-3, 0.02, 1.0, 300.0)] + [Q.tie_blocks()])
    d, n = Q.quantize(w)
    b = w.reshape(w.shape[0], -1, 32)
    assert (np.abs(b).max(axis=2) >= np.finfo(np.float32).tiny).all()
    q = n.astype(np.int32) - 8
    assert q.min() >= -7 and q.max() <= 7 and n.min() >= 1
    err = np.abs(b.astype(np.float64) - d[..., None].astype(np.float64) * q) / d[..., None].astype(np.float64)
    print("worst |w - w'| / d:", err.max())
    assert err.max() <= 0.5 + 2.0 ** -18
    assert (np.abs(q).max(axis=2) == 7).all()          # the largest weight of a block lands on +-7


def test_zero_and_non_finite_blocks_follow_the_rule():
    d, n = Q.quantize(Q.special_blocks())
    assert d[0, 0] == 0 and (n[0] == 8).all() and (Q.dequantize(d, n)[0] == 0).all()
    for i in (1, 2, 3):
        assert np.isnan(d[i, 0]) and (n[i] == 8).all()
        assert np.isnan(Q.dequantize(d, n)[i]).all()


def test_ties_round_to_even():
    t = Q.tie_blocks()
    d, n = Q.quantize(t)
    assert d[0, 0] == 1.0
    q = n[0, 0].astype(np.int32) - 8
    assert (q == np.clip(np.rint(t[0]), -7, 7)).all()
    assert q[1] == -6 and t[0, 1] == -6.5             # -6.5 -> -6 (even), its neighbour below -> -7
    assert q[2] == -7
