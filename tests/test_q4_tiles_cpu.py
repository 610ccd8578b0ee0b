"""(no GPU) where k_gemm_q4b3 keeps a nibble and what it makes of it, through the exported layout functions (csrc/gemm_q4_layout.h, stream_q4_layout.h):
the weight part of its LDS ring, the DMA lanes that fill it, the operand read, and the nibble -> bf16 conversion against the int8 kernel's."""
import ctypes as C
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import llama_go_amd as pkg
    L = C.CDLL(pkg.LIBLLAMAHIP)
    L.lh_gemm_q4_w_off.restype = L.lh_gemm_q4_read_off.restype = C.c_int64
    L.lh_gemm_q4_w_off.argtypes = [C.c_uint32] * 3
    L.lh_gemm_q4_read_off.argtypes = [C.c_uint32] * 4
    L.lh_gemm_q4_dma_lane.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32 * 2)]
    L.lh_stream_q4_operand.argtypes = [C.c_uint32, C.POINTER(C.c_uint32 * 4)]
    return L


W_BYTES = 2 * 2 * 256 * 16      # two slab pairs of [2][256 rows][16 B]


@pytest.mark.parametrize("slab0", [0, 2, 6, 344])
def test_w_stage_map_is_a_bijection(lib, slab0):
    """four consecutive slabs from an even one = the two live pairs: every byte of the ring's weight part exactly once; the pair after them reuses the first one's slot"""
    offs = [lib.lh_gemm_q4_w_off(slab0 + s, r, b) for s in range(4) for r in range(256) for b in range(16)]
    assert sorted(offs) == list(range(W_BYTES))
    assert lib.lh_gemm_q4_w_off(slab0 + 4, 77, 3) == lib.lh_gemm_q4_w_off(slab0, 77, 3)
    assert lib.lh_gemm_q4_w_off(0, 256, 0) == -1 and lib.lh_gemm_q4_w_off(0, 0, 16) == -1


@pytest.mark.parametrize("pair", [0, 1, 5])
def test_dma_lanes_land_at_base_plus_16_lane_and_cover_the_pair(lib, pair):
    seen = set()
    for wave in range(8):
        out = (C.c_uint32 * 2)()
        dst = []
        for lane in range(64):
            assert lib.lh_gemm_q4_dma_lane(wave, lane, C.byref(out)) == 0
            row, gran = out[0], out[1]
            assert row // 32 == wave and gran in (0, 1)           # a wave fetches its own 32 rows; source bytes 16 gran .. + 15 of the row's 32
            dst.append(lib.lh_gemm_q4_w_off(2 * pair + gran, row, 0))
            seen.add((row, gran))
        assert dst == [dst[0] + 16 * lane for lane in range(64)] and dst[0] % 16 == 0
    assert seen == set(itertools.product(range(256), (0, 1)))


def test_operand_read_finds_its_columns_and_spreads_over_the_banks(lib):
    rng = np.random.default_rng(4)
    nib = rng.integers(0, 16, (4, 256, 32), dtype=np.uint8)                         # [slab][row][column]
    lds = np.zeros(W_BYTES, np.uint8)
    for s, r, b in itertools.product(range(4), range(256), range(16)):
        lds[lib.lh_gemm_q4_w_off(s, r, b)] = nib[s, r, 2 * b] | (nib[s, r, 2 * b + 1] << 4)   # the nibble plane's byte: column 2 b low, 2 b + 1 high
    for s, wave in itertools.product(range(4), range(8)):
        banks = np.zeros(64, int)
        for lane in range(64):
            li, lh = lane & 31, lane >> 5
            off = lib.lh_gemm_q4_read_off(s, wave, li, lh)
            assert off % 8 == 0
            for st in range(2):
                dword = int.from_bytes(lds[off + 4 * st:off + 4 * st + 4].tobytes(), "little")
                assert [(dword >> (4 * e)) & 15 for e in range(8)] == nib[s, 32 * wave + li, 16 * lh + 8 * st:16 * lh + 8 * st + 8].tolist()
                banks[(off // 4 + st) % 64] += 1
        assert banks.max() <= 2, (s, wave, banks)


def test_conversion_equals_the_int8_kernels_for_every_byte(lib):
    """lh_stream_q4_operand over a reader dword against k_gemm_q8b3's convert of the expanded quants: element k = the high half of (float)(n_k - 8)"""
    out = (C.c_uint32 * 4)()
    for byte in range(256):
        for pos in range(4):
            other = (0x5A + 37 * byte) & 0xFF
            v = sum((byte if p == pos else other) << (8 * p) for p in range(4))
            lib.lh_stream_q4_operand(v, C.byref(out))
            q = np.array([((v >> (4 * k)) & 15) - 8 for k in range(8)], np.int8)     # k_expand_q4's quants
            want = (q.astype(np.float32).view(np.uint32) >> 16).astype(np.uint32)      # int8 -> fp32 -> its bf16 (exact: |q| <= 8)
            got = [(out[k // 2] >> (16 * (k & 1))) & 0xFFFF for k in range(8)]
            assert got == want.tolist(), (hex(v), got, want)
