"""not-gpu: the host side of lh_ctx_set_f16_stream (f16 models on the stream kernels, csrc/kernels_stream_f16.h; DESIGN 3k "Native stream kernels").

1. the libraries export the switch's entries and the headers declare them;
2. the weight image of k_stream_dma_h (csrc/stream_f16_layout.h, exported as lh_stream_f16_image_off / lh_stream_f16_read_off - the functions the kernel's
   loader waves and MFMA waves both call) for both chunk lengths and every row-tile count built:
     * (image row, 16-byte granule) -> offset is a bijection onto the image, and equals the lane-linear destination of the loader's LDS-DMA pieces;
     * the address an MFMA lane (tile, r16, k-block, slot) reads holds exactly the halves of columns 16 kb + 4 slot .. + 3 of its row;
     * under the LDS bank model (ds_read_b64: two 32-lane halves, bank (address / 4) % 64) every operand read the MFMA waves issue is conflict-free;
3. the same layout behind its own main (tests/stream_f16_layout_main.cpp) built with -fsanitize=address,undefined, as a child process: the image is a heap
   block of exactly its size there.
(A setter / getter round trip needs a context, and lh_ctx_create needs a device: tests/test_gpu_f16_stream.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCS = (64, 128)
MAXTS = (1, 2, 3, 4, 6, 8)          # stream_maxt_built, csrc/plan.hip


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    lib.lh_stream_f16_image_off.restype = C.c_int64
    lib.lh_stream_f16_image_off.argtypes = [C.c_uint32] * 3
    lib.lh_stream_f16_read_off.restype = C.c_int64
    lib.lh_stream_f16_read_off.argtypes = [C.c_uint32] * 5
    return lib


def test_entries_are_exported_and_declared(built):
    import llama_go_amd as pkg
    hip, go = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL), C.CDLL(pkg.LIBLLAMAGO)
    hdr = open(os.path.join(ROOT, "include", "llamahip.h")).read()
    ext = open(os.path.join(ROOT, "include", "llamago_ext.h")).read()
    for name in ("lh_ctx_set_f16_stream", "lh_ctx_f16_stream", "lh_stream_f16_image_off", "lh_stream_f16_read_off"):
        assert hasattr(hip, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("llamago_SetF16Stream", "llamago_F16Stream", "llamago_BatchSetF16Stream", "llamago_BatchF16Stream"):
        assert hasattr(go, name), name
        assert re.search(r"\b" + name + r"\s*\(", ext), name
    # a NULL context: the setter refuses, the getter says off
    hip.lh_ctx_set_f16_stream.argtypes = [C.c_void_p, C.c_int]
    hip.lh_ctx_f16_stream.argtypes = [C.c_void_p]
    assert hip.lh_ctx_set_f16_stream(None, 1) == -1 and hip.lh_ctx_f16_stream(None) == 0
    from llama_go_amd import mlapi
    assert hasattr(mlapi.Context, "SetF16Stream") and hasattr(mlapi.Batch, "SetF16Stream")
    assert isinstance(mlapi.Context.f16_stream, property) and isinstance(mlapi.Batch.f16_stream, property)


def test_arguments_out_of_range_are_refused(lib):
    assert lib.lh_stream_f16_image_off(32, 0, 0) == -1 and lib.lh_stream_f16_image_off(64, 128, 0) == -1
    assert lib.lh_stream_f16_image_off(64, 0, 8) == -1 and lib.lh_stream_f16_image_off(128, 0, 16) == -1
    assert lib.lh_stream_f16_read_off(64, 8, 0, 0, 0) == -1 and lib.lh_stream_f16_read_off(64, 0, 16, 0, 0) == -1
    assert lib.lh_stream_f16_read_off(64, 0, 0, 4, 0) == -1 and lib.lh_stream_f16_read_off(128, 0, 0, 8, 0) == -1 and lib.lh_stream_f16_read_off(128, 0, 0, 0, 4) == -1


@pytest.mark.parametrize("kc", KCS)
def test_image_is_a_bijection_and_the_reader_finds_its_halves(lib, kc):
    grw, rpw = kc // 8, 64 // (kc // 8)          # granules per row; rows per 1 KB piece
    for maxt in MAXTS:
        rows = maxt * 16
        size = rows * kc * 2
        img = [None] * (size // 2)               # one entry per half: (row, column)
        seen = set()
        for r in range(rows):
            for g in range(grw):
                off = lib.lh_stream_f16_image_off(kc, r, g)
                assert 0 <= off <= size - 16 and off % 16 == 0 and off not in seen, (kc, maxt, r, g, off)
                assert off // (kc * 2) == r                        # a granule stays in its own row (the DMA pieces cover whole rows)
                seen.add(off)
                for e in range(8):
                    img[off // 2 + e] = (r, g * 8 + e)
        assert len(seen) == size // 16
        # the loader: piece q, lane i lands at q * 1024 + 16 i = position i % grw of row q * rpw + i // grw, and picks the source granule stored there
        for q in range(rows // rpw):
            for lane in range(64):
                r, gd = q * rpw + lane // grw, lane % grw
                src = [g for g in range(grw) if lib.lh_stream_f16_image_off(kc, r, g) == q * 1024 + lane * 16]
                assert len(src) == 1
                assert lib.lh_stream_f16_image_off(kc, r, gd) == r * kc * 2 + src[0] * 16      # an involution: pos(r, pos(r, g)) = g
        for t in range(maxt):
            for r16 in range(16):
                for kb in range(kc // 16):
                    for slot in range(4):
                        off = lib.lh_stream_f16_read_off(kc, t, r16, kb, slot)
                        assert off % 8 == 0 and 0 <= off <= size - 8
                        assert img[off // 2:off // 2 + 4] == [(t * 16 + r16, 16 * kb + 4 * slot + e) for e in range(4)], (kc, maxt, t, r16, kb, slot)


@pytest.mark.parametrize("kc", KCS)
def test_operand_reads_are_conflict_free_under_the_bank_model(lib, kc):
    """One ds_read_b64 of an MFMA wave: lane l = (r16 = l & 15, slot = l >> 4) reads 8 bytes of (tile t, k-block kb).  Each 32-lane half must touch
    64 different banks (32 lanes x 2 banks)."""
    for t in range(max(MAXTS)):
        for kb in range(kc // 16):
            for half in (0, 1):
                banks = []
                for lane in range(32 * half, 32 * half + 32):
                    off = lib.lh_stream_f16_read_off(kc, t, lane & 15, kb, lane >> 4)
                    banks += [(off // 4) % 64, (off // 4 + 1) % 64]
                assert len(set(banks)) == 64, (kc, t, kb, half, sorted(banks))


def test_layout_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stream_f16_layout_main")
    # the runtimes are linked statically: the child then starts whatever its environment preloads, and the environment is passed on as it is
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
           os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stream_f16_layout_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]
    cases = [(kc, maxt) for kc in KCS for maxt in MAXTS]
    r = subprocess.run([exe], input="".join(f"{kc} {maxt}\n" for kc, maxt in cases), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines() == [f"{kc} {maxt} ok" for kc, maxt in cases]
