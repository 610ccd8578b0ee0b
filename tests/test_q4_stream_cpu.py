"""not-gpu: the host side of lh_ctx_set_q4_stream (block-int4 models on the bf16 stream kernel, csrc/kernels_stream_q4b.h; DESIGN 3l "Native stream kernel").

1. the libraries export the switch's entries and the headers declare them; a NULL context: the setter refuses (-1), the getter says off (0);
2. the weight image of k_stream_q4b (csrc/stream_q4_layout.h, exported as lh_stream_q4_image_off / lh_stream_q4_read_off - the functions the kernel's
   DMA side and reading side both call) for the three chunk lengths and every row-tile count built:
     * (image row, 16-byte granule) -> offset is a bijection onto the weight part of the image, and equals the lane-linear destination of the DMA pieces;
     * the four bytes an MFMA lane (tile, r16, quant block, slot) reads are exactly the bytes of columns 32 kb + 8 slot .. + 7 of its row;
     * under the LDS bank model of tests/test_f16_stream_cpu.py (bank = (address / 4) % 64; the wave's ds_read_b32 - one dword per lane - judged as it is
       issued: the two 32-lane halves, and here also the 64 lanes together) every operand read is conflict-free;
3. the kernel's nibble -> bf16 conversion on the host (lh_stream_q4_operand): for all 256 byte values the high halves of (float)((b & 15) - 8) and
   (float)((b >> 4) - 8); for a few thousand dwords the operand k_stream_q8b's conversion yields for the eight expanded int8 quants, element by element;
4. the same layout and conversion behind their own main (tests/stream_q4_layout_main.cpp) built with -fsanitize=address,undefined, as a child process:
   the image is a heap block of exactly its size there.
(A setter / getter round trip needs a context, and lh_ctx_create needs a device: tests/test_gpu_q4_stream.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCS = (128, 256, 512)
MAXTS = (1, 2, 3, 4, 6, 8)          # stream_maxt_built, csrc/plan.hip


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    lib.lh_stream_q4_image_off.restype = C.c_int64
    lib.lh_stream_q4_image_off.argtypes = [C.c_uint32] * 3
    lib.lh_stream_q4_read_off.restype = C.c_int64
    lib.lh_stream_q4_read_off.argtypes = [C.c_uint32] * 5
    lib.lh_stream_q4_operand.restype = None
    lib.lh_stream_q4_operand.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
    return lib


def test_entries_are_exported_and_declared(built):
    import llama_go_amd as pkg
    hip, go = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL), C.CDLL(pkg.LIBLLAMAGO)
    hdr = open(os.path.join(ROOT, "include", "llamahip.h")).read()
    ext = open(os.path.join(ROOT, "include", "llamago_ext.h")).read()
    for name in ("lh_ctx_set_q4_stream", "lh_ctx_q4_stream", "lh_stream_q4_image_off", "lh_stream_q4_read_off", "lh_stream_q4_operand"):
        assert hasattr(hip, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("llamago_SetQ4Stream", "llamago_Q4Stream", "llamago_BatchSetQ4Stream", "llamago_BatchQ4Stream"):
        assert hasattr(go, name), name
        assert re.search(r"\b" + name + r"\s*\(", ext), name
    # a NULL context: the setter refuses, the getter says off
    hip.lh_ctx_set_q4_stream.argtypes = [C.c_void_p, C.c_int]
    hip.lh_ctx_q4_stream.argtypes = [C.c_void_p]
    assert hip.lh_ctx_set_q4_stream(None, 1) == -1 and hip.lh_ctx_q4_stream(None) == 0
    from llama_go_amd import mlapi
    assert hasattr(mlapi.Context, "SetQ4Stream") and hasattr(mlapi.Batch, "SetQ4Stream")
    assert isinstance(mlapi.Context.q4_stream, property) and isinstance(mlapi.Batch.q4_stream, property)
    go_src = open(os.path.join(ROOT, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    assert "C.lh_ctx_set_q4_stream(" in go_src and "C.lh_ctx_q4_stream(" in go_src


def test_arguments_out_of_range_are_refused(lib):
    assert lib.lh_stream_q4_image_off(64, 0, 0) == -1 and lib.lh_stream_q4_image_off(1024, 0, 0) == -1 and lib.lh_stream_q4_image_off(128, 128, 0) == -1
    assert lib.lh_stream_q4_image_off(128, 0, 4) == -1 and lib.lh_stream_q4_image_off(256, 0, 8) == -1 and lib.lh_stream_q4_image_off(512, 0, 16) == -1
    assert lib.lh_stream_q4_read_off(64, 0, 0, 0, 0) == -1 and lib.lh_stream_q4_read_off(128, 8, 0, 0, 0) == -1 and lib.lh_stream_q4_read_off(128, 0, 16, 0, 0) == -1
    assert lib.lh_stream_q4_read_off(128, 0, 0, 4, 0) == -1 and lib.lh_stream_q4_read_off(512, 0, 0, 16, 0) == -1 and lib.lh_stream_q4_read_off(256, 0, 0, 0, 4) == -1
    assert lib.lh_stream_q4_image_off(512, 127, 15) >= 0 and lib.lh_stream_q4_read_off(512, 7, 15, 15, 3) >= 0


@pytest.mark.parametrize("kc", KCS)
def test_image_is_a_bijection_and_the_reader_finds_its_bytes(lib, kc):
    grw, rpw, pitch = kc // 32, 64 // (kc // 32), kc // 2      # granules per row; rows per 1 KB piece; bytes per row
    for maxt in MAXTS:
        rows = maxt * 16
        size = rows * pitch
        img = [None] * size                       # one entry per byte: (row, byte of the row's chunk = columns 2 b, 2 b + 1)
        seen = set()
        for r in range(rows):
            for g in range(grw):
                off = lib.lh_stream_q4_image_off(kc, r, g)
                assert 0 <= off <= size - 16 and off % 16 == 0 and off not in seen, (kc, maxt, r, g, off)
                assert off // pitch == r                           # a granule stays in its own row (the DMA pieces cover whole rows)
                seen.add(off)
                for e in range(16):
                    img[off + e] = (r, g * 16 + e)
        assert len(seen) == size // 16
        # the DMA side: piece q, lane i lands at q * 1024 + 16 i = position i % grw of row q * rpw + i // grw, and picks the source granule stored there
        assert (rows // rpw) * 1024 == size
        for q in range(rows // rpw):
            for lane in range(64):
                r, gd = q * rpw + lane // grw, lane % grw
                src = [g for g in range(grw) if lib.lh_stream_q4_image_off(kc, r, g) == q * 1024 + lane * 16]
                assert len(src) == 1
                assert lib.lh_stream_q4_image_off(kc, r, gd) == r * pitch + src[0] * 16      # an involution: pos(r, pos(r, g)) = g
        for t in range(maxt):
            for r16 in range(16):
                for kb in range(kc // 32):
                    for slot in range(4):
                        off = lib.lh_stream_q4_read_off(kc, t, r16, kb, slot)
                        assert off % 4 == 0 and 0 <= off <= size - 4
                        # byte b of a row's chunk = columns 2 b, 2 b + 1: columns 32 kb + 8 slot .. + 7 are bytes 16 kb + 4 slot .. + 3
                        assert img[off:off + 4] == [(t * 16 + r16, 16 * kb + 4 * slot + e) for e in range(4)], (kc, maxt, t, r16, kb, slot)


@pytest.mark.parametrize("kc", KCS)
def test_operand_reads_are_conflict_free_under_the_bank_model(lib, kc):
    """One ds_read_b32 of a wave: lane l = (r16 = l & 15, slot = l >> 4) reads 4 bytes of (tile t, quant block kb): 256 bytes, one 16-byte granule from
    each of 16 rows.  The 64 lanes must touch the 64 banks once each - and so does each 32-lane half, the unit the instruction is issued in."""
    for t in range(max(MAXTS)):
        for kb in range(kc // 32):
            banks = [(lib.lh_stream_q4_read_off(kc, t, lane & 15, kb, lane >> 4) // 4) % 64 for lane in range(64)]
            assert sorted(banks) == list(range(64)), (kc, t, kb, sorted(banks))
            for half in (0, 1):
                assert len(set(banks[32 * half:32 * half + 32])) == 32, (kc, t, kb, half)


def operand(lib, v):
    out = (C.c_uint32 * 4)()
    lib.lh_stream_q4_operand(C.c_uint32(v), out)
    return [int(x) for x in out]


def bf16_of_int(q):
    """the high half of (float)q"""
    return int(np.array([q], np.float32).view(np.uint32)[0]) >> 16


def test_conversion_of_every_byte_value(lib):
    for b in range(256):
        o = operand(lib, b)                      # nibbles 0 and 1 of the dword
        assert o[0] & 0xffff == bf16_of_int((b & 15) - 8) and o[0] >> 16 == bf16_of_int((b >> 4) - 8), (b, hex(o[0]))
        assert o[1:] == [bf16_of_int(-8) * 0x10001] * 3, (b, o)                   # the six nibbles 0 around it
        for byte in (1, 2, 3):                   # the same byte in the dword's other three places
            o = operand(lib, b << (8 * byte))
            assert o[byte] & 0xffff == bf16_of_int((b & 15) - 8) and o[byte] >> 16 == bf16_of_int((b >> 4) - 8), (b, byte, hex(o[byte]))


def q8b_operand(quants):
    """k_stream_q8b's conversion of eight int8 quants (csrc/kernels_stream_q8b.h): (float)q exact, its high half IS the bf16; v_perm_b32 0x07060302 packs
    the high halves of elements 2 j (low) and 2 j + 1 (high)"""
    f = np.asarray(quants, np.int8).astype(np.float32).view(np.uint32)
    return [int((f[2 * j] >> 16) | (f[2 * j + 1] & 0xffff0000)) for j in range(4)]


def expand_q4(v):
    """k_expand_q4's step on one dword (csrc/kernels_q4.h): the int8 quants n - 8 of its eight nibbles, in column order"""
    lo = (((v & 0x0f0f0f0f) + 0x78787878) ^ 0x80808080) & 0xffffffff
    hi = ((((v >> 4) & 0x0f0f0f0f) + 0x78787878) ^ 0x80808080) & 0xffffffff
    out = []
    for b in range(4):
        out += [(lo >> (8 * b)) & 0xff, (hi >> (8 * b)) & 0xff]
    return np.array(out, np.uint8).view(np.int8)


def test_conversion_equals_the_int8_kernels_on_the_expanded_quants(lib):
    rng = np.random.default_rng(4)
    dwords = [0x00000000, 0xffffffff, 0x80808080, 0x08080808, 0x76543210, 0xfedcba98] + [int(x) for x in rng.integers(0, 2 ** 32, 4000, dtype=np.uint64)]
    for v in dwords:
        q = expand_q4(v)
        assert [int(x) for x in q] == [((v >> (4 * k)) & 15) - 8 for k in range(8)], hex(v)
        assert operand(lib, v) == q8b_operand(q), hex(v)


def test_layout_and_conversion_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stream_q4_layout_main")
    # the runtimes are linked statically: the child then starts whatever its environment preloads, and the environment is passed on as it is
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
           os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stream_q4_layout_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]
    cases = [(kc, maxt) for kc in KCS for maxt in MAXTS]
    r = subprocess.run([exe], input="".join(f"{kc} {maxt}\n" for kc, maxt in cases), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines() == [f"{kc} {maxt} ok" for kc, maxt in cases] + ["convert ok"]
