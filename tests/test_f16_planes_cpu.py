"""not-gpu: the ring image and the product list of k_stream_b9_h (csrc/stream_b9h_layout.h, exported as lh_stream_b9h_piece / _read_off / _product - the
functions the kernel's loader waves and MFMA waves call; DESIGN 3k "Native planes kernel").  (The split's exactness: tests/test_f16_tiles_cpu.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILT = [(maxt, nct) for maxt in (1, 2, 3, 4, 6, 8) for nct in (1, 2, 3, 4) if not (maxt == 8 and nct == 4)]   # stream_maxt_built / launch_stream_b9, csrc/plan.hip
# k_stream_b9 at B9S_PRODUCTS = 8 (csrc/kernels_stream_b9.h: rows 1..8 of PX / PW): (activation plane, weight part), 0 hi, 1 mid, 2 lo
EIGHT = [(2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    lib.lh_stream_b9h_piece.restype = C.c_int
    lib.lh_stream_b9h_piece.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)]
    lib.lh_stream_b9h_read_off.restype = C.c_int64
    lib.lh_stream_b9h_read_off.argtypes = [C.c_uint32, C.c_uint32, C.c_int] + [C.c_uint32] * 4
    lib.lh_stream_b9h_product.restype = C.c_int
    lib.lh_stream_b9h_product.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


@pytest.mark.parametrize("maxt,nct", BUILT)
def test_pieces_cover_the_image_once_and_reads_find_their_columns(lib, maxt, nct):
    size, out = maxt * 2048 + nct * 6144, (C.c_uint32 * 4)()
    img = {}
    for q in range(2 * maxt + 6 * nct):
        base = None
        for lane in range(64):
            assert lib.lh_stream_b9h_piece(maxt, nct, q, lane, out) == 0
            dst, kind, row, gran = (int(v) for v in out)
            base = dst if lane == 0 else base
            assert dst == base + 16 * lane and dst + 16 <= size and dst not in img, (q, lane)
            assert gran < 8 and (row < nct * 16 if kind else row >> 4 == q >> 1), (q, lane)      # a weight piece lies inside one 16-row tile
            img[dst] = (kind, row, gran)
    assert len(img) * 16 == size
    for kb in range(2):
        for slot in range(4):
            for r16 in range(16):
                for t in range(maxt):
                    assert img[lib.lh_stream_b9h_read_off(maxt, nct, -1, t, r16, kb, slot)] == (0, t * 16 + r16, kb * 4 + slot)
                for p in range(3):
                    for c in range(nct):
                        assert img[lib.lh_stream_b9h_read_off(maxt, nct, p, c, r16, kb, slot)] == (1 + p, c * 16 + r16, kb * 4 + slot)
    assert lib.lh_stream_b9h_piece(maxt, nct, 2 * maxt + 6 * nct, 0, out) == -1 and lib.lh_stream_b9h_read_off(maxt, nct, -1, maxt, 0, 0, 0) == -1


def test_six_products_are_the_eight_without_wl_in_order(lib):
    out = (C.c_int * 2)()

    def products(n):
        res = []
        for i in range(n):
            assert lib.lh_stream_b9h_product(n, i, out) == 0
            res.append((out[0], out[1]))
        return res
    assert products(8) == EIGHT
    assert products(6) == [p for p in EIGHT if p[1] != 2]


def test_layout_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stream_b9h_layout_main")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
           os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stream_b9h_layout_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], input="".join(f"{maxt} {nct}\n" for maxt, nct in BUILT), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines() == [f"{maxt} {nct} ok" for maxt, nct in BUILT]
