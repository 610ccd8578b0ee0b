"""not-gpu: the ring image and the product list of k_stream_b9w_h (csrc/stream_b9wh_layout.h, exported as lh_stream_b9wh_piece / _read_off - the functions
the kernel's loader waves and MFMA waves call; the products are lh_stream_b9h_product's, which the kernel shares; DESIGN 3k "Native wide planes kernel")."""
import ctypes as C

import pytest

BUILT = [(maxt, nct) for maxt in (1, 2, 3, 4, 6, 8) for nct in (5, 6, 7, 8)]   # b9wh_built == b9w_built, csrc/stream_b9w_layout.h
# k_stream_b9w at NPROD = 8 (csrc/kernels_stream_b9w.h: entries 1..8 of PX / PW): (activation plane, weight part), 0 hi, 1 mid, 2 lo
EIGHT = [(2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    lib.lh_stream_b9wh_piece.restype = C.c_int
    lib.lh_stream_b9wh_piece.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)]
    lib.lh_stream_b9wh_read_off.restype = C.c_int64
    lib.lh_stream_b9wh_read_off.argtypes = [C.c_uint32, C.c_uint32, C.c_int] + [C.c_uint32] * 4
    lib.lh_stream_b9h_product.restype = C.c_int
    lib.lh_stream_b9h_product.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


@pytest.mark.parametrize("maxt,nct", BUILT)
def test_pieces_cover_the_image_once_and_reads_find_their_columns(lib, maxt, nct):
    size, pieces, out = maxt * 2048 + nct * 6144, 2 * maxt + 6 * nct, (C.c_uint32 * 4)()
    img = {}
    for q in range(pieces):
        base = None
        for lane in range(64):
            assert lib.lh_stream_b9wh_piece(maxt, nct, q, lane, out) == 0
            dst, kind, row, gran = (int(v) for v in out)
            base = dst if lane == 0 else base
            assert dst == base + 16 * lane and dst % 16 == 0 and dst + 16 <= size and dst not in img, (q, lane)
            assert gran < 8 and (row < nct * 16 if kind else row >> 4 == q >> 1), (q, lane)      # a weight piece lies inside one 16-row tile
            assert (kind == 0) == (dst < maxt * 2048), (q, lane)                                  # the planes follow the weights
            img[dst] = (kind, row, gran)
    assert len(img) * 16 == size
    for kb in range(2):
        for slot in range(4):
            for r16 in range(16):
                for t in range(maxt):
                    assert img[lib.lh_stream_b9wh_read_off(maxt, nct, -1, t, r16, kb, slot)] == (0, t * 16 + r16, kb * 4 + slot)
                for p in range(3):
                    for c in range(nct):
                        assert img[lib.lh_stream_b9wh_read_off(maxt, nct, p, c, r16, kb, slot)] == (1 + p, c * 16 + r16, kb * 4 + slot)
    assert lib.lh_stream_b9wh_piece(maxt, nct, pieces, 0, out) == -1
    assert lib.lh_stream_b9wh_read_off(maxt, nct, -1, maxt, 0, 0, 0) == -1 and lib.lh_stream_b9wh_read_off(maxt, nct, 0, nct, 0, 0, 0) == -1


def test_six_products_are_the_eight_without_wl_in_order(lib):
    out = (C.c_int * 2)()
    products = lambda n: [(lib.lh_stream_b9h_product(n, i, out), out[0], out[1]) for i in range(n)]   # noqa: E731
    assert products(8) == [(0,) + p for p in EIGHT]
    assert products(6) == [(0,) + p for p in EIGHT if p[1] != 2]
