"""not-gpu: the weight part of a ring image of k_stream_dma_q41 (csrc/stream_q41_layout.h through the lh_stream_q41_* exports - the functions the kernel's
loader waves and MFMA waves both call; DESIGN 3m "Native stream kernels").  A chunk of kc columns of a weight row is kc / 32 nibble granules (16 bytes = one
quant block, byte b = columns 2 b | 2 b + 1) and kc / 64 pair granules (16 bytes = (d, m) of blocks 2 c, 2 c + 1)."""
import ctypes as C

import pytest

U = C.c_uint32


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    for name, n in (("weight_bytes", 2), ("granule_off", 5), ("read_off", 6), ("pair_off", 5)):
        f = getattr(lib, "lh_stream_q41_" + name)
        f.restype, f.argtypes = C.c_int64, [U] * n
    lib.lh_stream_q41_granule_src.restype, lib.lh_stream_q41_granule_src.argtypes = C.c_int, [U, U, U, C.POINTER(U * 3)]
    return lib


def image(lib, kc, maxt):
    """the loader's placement: {byte offset: what it holds} - ('n', row, column pair index) per nibble byte, ('p', row, block, 0 d | 1 m, byte) per pair byte"""
    gn, gp = kc // 32, kc // 64
    total = maxt * 16 * (gn + gp)
    size = lib.lh_stream_q41_weight_bytes(kc, maxt)
    assert size % 1024 == 0 and 0 <= size - total * 16 < 1024                 # whole LDS-DMA instructions, less than one of padding
    img, out = {}, (U * 3)()
    for pos in range(total):                                                  # lane pos % 64 of instruction pos // 64 lands at 16 pos
        assert lib.lh_stream_q41_granule_src(kc, maxt, pos, C.byref(out)) == 0
        plane, r, g = out
        assert plane < 2 and r < maxt * 16 and g < (gp if plane else gn)
        assert lib.lh_stream_q41_granule_off(kc, maxt, plane, r, g) == 16 * pos, (kc, maxt, pos)   # loader and reader agree
        for b in range(16):
            img[16 * pos + b] = ("p", r, 2 * g + b // 8, (b % 8) // 4, b % 4) if plane else ("n", r, 16 * g + b)
    assert lib.lh_stream_q41_granule_src(kc, maxt, total, C.byref(out)) == -1
    return img, total


@pytest.mark.parametrize("maxt", [1, 6])
@pytest.mark.parametrize("kc", [64, 128])
def test_placement_is_a_bijection_and_the_reader_finds_its_bytes(lib, kc, maxt):
    img, total = image(lib, kc, maxt)
    assert len(img) == 16 * total and len(set(img.values())) == 16 * total    # onto the weight part, nothing twice
    assert {v[:2] for v in img.values()} == {(p, r) for p in "np" for r in range(maxt * 16)}
    for t in range(maxt):
        for r16 in range(16):
            for kb in range(kc // 16):
                pair = lib.lh_stream_q41_pair_off(kc, maxt, t, r16, kb)
                assert pair % 8 == 0 and [img[pair + b] for b in range(8)] == [("p", t * 16 + r16, kb >> 1, b // 4, b % 4) for b in range(8)]
                for slot in range(4):
                    off = lib.lh_stream_q41_read_off(kc, maxt, t, r16, kb, slot)
                    assert off % 4 == 2 * (slot & 1)                          # half slot & 1 of an aligned dword
                    assert [img[off], img[off + 1]] == [("n", t * 16 + r16, 8 * kb + 2 * slot + e) for e in (0, 1)], (kc, maxt, t, r16, kb, slot)


@pytest.mark.parametrize("maxt", [1, 6])
@pytest.mark.parametrize("kc", [64, 128])
def test_operand_reads_are_conflict_free_under_the_bank_model(lib, kc, maxt):
    """64 banks of 4 bytes, a read served per half-wave (32 lanes: 16 rows x two slots); lanes may share an ADDRESS, different addresses must not share a
    bank.  The nibble read is the aligned dword (ds_read_b32), the pair read 8 bytes (ds_read_b64)."""
    for t in range(maxt):
        for kb in range(kc // 16):
            for half in (0, 1):
                lanes = range(32 * half, 32 * half + 32)
                nib = {lib.lh_stream_q41_read_off(kc, maxt, t, l & 15, kb, l >> 4) & ~3 for l in lanes}
                pair = {lib.lh_stream_q41_pair_off(kc, maxt, t, l & 15, kb) for l in lanes}
                assert len(nib) == 16 and len({(a // 4) % 64 for a in nib}) == 16, (kc, t, kb, half)
                assert len(pair) == 16 and len({(a // 4 + i) % 64 for a in pair for i in (0, 1)}) == 32, (kc, t, kb, half)
