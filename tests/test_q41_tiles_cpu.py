"""(no GPU) csrc/gemm_q41_layout.h through its exports: over all 512 lanes and two slabs k_gemm_b9_q41's DMA destinations are a bijection onto the stage's
nibble part / a pair slot, and the operand read returns the row and the bytes the DMA put there."""
import ctypes as C

import numpy as np
import pytest

W_OFF, STAGE, SLOT = 3 * 128 * 64, 3 * 128 * 64 + 256 * 16, 256 * 16


@pytest.fixture(scope="module")
def lib():
    import llama_go_amd as pkg
    return C.CDLL(pkg.LIBLLAMAHIP)


def test_dma_and_operand_read_meet(lib):
    rng = np.random.default_rng(1)
    nib = rng.integers(0, 256, (2, 256, 16), dtype=np.uint8)         # [slab][tile row][byte]: the nibble plane's granules
    pairs = rng.standard_normal((256, 4)).astype(np.float32)         # [tile row](d0, m0, d1, m1): one slab pair
    stage, slot = np.zeros((2, STAGE), np.uint8), np.zeros(SLOT, np.uint8)
    seen_n, seen_p, out = set(), set(), (C.c_uint32 * 3)()
    for q in range(4):                                               # 4 pieces x 64 lanes = the tile's 256 rows, per slab (nibbles) / per pair
        for lane in range(64):
            assert lib.lh_gemm_q41_piece(q, lane, C.byref(out)) == 0
            row, nd, pd = out
            assert row < 256 and W_OFF <= nd and nd + 16 <= STAGE and pd + 16 <= SLOT and nd % 16 == 0 and pd % 16 == 0
            assert nd == W_OFF + 1024 * q + 16 * lane and pd == 1024 * q + 16 * lane      # what the instruction does: base + 16 lane
            seen_n.add(nd); seen_p.add(pd)
            stage[0, nd:nd + 16], stage[1, nd:nd + 16] = nib[0, row], nib[1, row]
            slot[pd:pd + 16] = pairs[row].view(np.uint8)
    assert len(seen_n) == 256 and len(seen_p) == 256                 # bijective: every granule of the 4 KB written once
    ro = (C.c_uint32 * 2)()
    for wave in range(8):
        for li in range(32):
            assert lib.lh_gemm_q41_read_off(wave, li, C.byref(ro)) == 0
            r = 32 * wave + li
            for s in range(2):
                assert bytes(stage[s, ro[0]:ro[0] + 16]) == bytes(nib[s, r])              # dword 2 kk + lh: columns 16 kk + 8 lh .. + 7
            assert bytes(slot[ro[1]:ro[1] + 16]) == pairs[r].tobytes()
    assert lib.lh_gemm_q41_piece(4, 0, C.byref(out)) == -1 and lib.lh_gemm_q41_read_off(0, 32, C.byref(ro)) == -1
