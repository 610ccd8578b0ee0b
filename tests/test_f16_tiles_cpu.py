"""not-gpu: the host side of lh_ctx_set_f16_tiles (f16 models on the bf16 tile GEMM, csrc/kernels_gemm_f16.h; DESIGN 3k "Native tile GEMM").

1. the libraries export the switch's entries and the pure pieces of k_gemm_b9_h, and the headers declare them;
2. the weight split (csrc/gemm_f16_layout.h gemm_h_split, exported as lh_gemm_f16_split - the function the kernel calls per half) over all 65 536
   patterns.  For every finite half: the parts equal split3 (csrc/kernels_common.h) of the widened value, restated in numpy; the third part is +0; hi + mid
   is the value; every non-zero part is >= 2^-100 (split_exact_values' range - the smallest is 2^-24);
3. the ring stage: the 40 DMA pieces of a slab (lh_gemm_f16_piece) cover the stage's 40 960 bytes exactly once, five per wave with no surplus slot; the
   swizzle is a bijection per group of four rows; a lane's weight read (lh_gemm_f16_w_read_off) finds the granule of its k-step and is conflict-free under
   the LDS bank model of a ds_read_b128;
4. the same header behind its own main (tests/gemm_f16_split_main.cpp) built with -fsanitize=address,undefined, as a child process.
(A setter / getter round trip needs a context, and lh_ctx_create needs a device: tests/test_gpu_f16_tiles.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE, W_OFF, XP = 40960, 24576, 8192


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    lib.lh_gemm_f16_split.restype = None
    lib.lh_gemm_f16_split.argtypes = [C.c_uint16, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.lh_gemm_f16_piece.restype = C.c_int
    lib.lh_gemm_f16_piece.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32 * 3)]
    lib.lh_gemm_f16_w_read_off.restype = C.c_int64
    lib.lh_gemm_f16_w_read_off.argtypes = [C.c_uint32] * 4
    return lib


def test_entries_are_exported_and_declared(built):
    import llama_go_amd as pkg
    hip, go = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL), C.CDLL(pkg.LIBLLAMAGO)
    hdr = open(os.path.join(ROOT, "include", "llamahip.h")).read()
    ext = open(os.path.join(ROOT, "include", "llamago_ext.h")).read()
    for name in ("lh_ctx_set_f16_tiles", "lh_ctx_f16_tiles", "lh_gemm_f16_split", "lh_gemm_f16_piece", "lh_gemm_f16_w_read_off"):
        assert hasattr(hip, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("llamago_SetF16Tiles", "llamago_F16Tiles"):
        assert hasattr(go, name), name
        assert re.search(r"\b" + name + r"\s*\(", ext), name
    # a NULL context: the setter refuses, the getter says off
    hip.lh_ctx_set_f16_tiles.argtypes = [C.c_void_p, C.c_int]
    hip.lh_ctx_f16_tiles.argtypes = [C.c_void_p]
    assert hip.lh_ctx_set_f16_tiles(None, 1) == -1 and hip.lh_ctx_f16_tiles(None) == 0
    from llama_go_amd import mlapi
    assert hasattr(mlapi.Context, "SetF16Tiles") and isinstance(mlapi.Context.f16_tiles, property)
    go_src = open(os.path.join(ROOT, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    assert "C.lh_ctx_set_f16_tiles(" in go_src and "C.lh_ctx_f16_tiles(" in go_src


def split3_numpy(x):
    """csrc/kernels_common.h split3 on finite fp32 values: three bf16 parts as uint16"""
    x = x.astype(np.float32)
    xb = x.view(np.uint32)
    h = xb & np.uint32(0xffff0000)
    r1 = (x - h.view(np.float32)).astype(np.float32)
    m = r1.view(np.uint32) & np.uint32(0xffff0000)
    r2 = (r1 - m.view(np.float32)).astype(np.float32)
    return (h >> 16).astype(np.uint16), (m >> 16).astype(np.uint16), (r2.view(np.uint32) >> 16).astype(np.uint16)


def test_split_of_every_half_pattern(lib):
    halves = np.arange(65536, dtype=np.uint16)
    w = np.zeros(65536, dtype=np.uint32)
    r1 = np.zeros(65536, dtype=np.uint32)
    a, b = C.c_uint32(), C.c_uint32()
    for h in range(65536):
        lib.lh_gemm_f16_split(h, C.byref(a), C.byref(b))
        w[h], r1[h] = a.value, b.value
    wide = halves.view(np.float16).astype(np.float32)
    finite = np.isfinite(wide)
    assert int(finite.sum()) == 63488
    # the widening is numpy's (exact, subnormals kept); inf / NaN widen to inf / NaN too (outside the kernel's contract, not split further here)
    assert (w[finite] == wide.view(np.uint32)[finite]).all()
    assert (np.isinf(w.view(np.float32)) == np.isinf(wide)).all() and (np.isnan(w.view(np.float32)) == np.isnan(wide)).all()
    hi, mid, lo = split3_numpy(wide[finite])
    kh, km = (w[finite] >> 16).astype(np.uint16), (r1[finite] >> 16).astype(np.uint16)      # what the kernel's byte-permute packs
    assert (kh == hi).all() and (km == mid).all()
    assert (lo == 0).all()                                   # the third part is +0 (bits, not just value): the plane k_gemm_b9_h never builds
    assert (r1[finite] & 0xffff == 0).all()                  # the remainder IS a bf16
    f = lambda p: (p.astype(np.uint32) << 16).view(np.float32)   # noqa: E731
    assert ((f(kh).astype(np.float64) + f(km).astype(np.float64)) == wide[finite].astype(np.float64)).all()
    parts = np.abs(np.concatenate([f(kh), f(km)]))
    nz = parts[parts != 0]
    assert float(nz.min()) == 2.0 ** -24 and float(nz.min()) >= 2.0 ** -100
    assert np.isfinite(parts).all()


def pieces(lib):
    out = {}
    buf = (C.c_uint32 * 3)()
    for p in range(40):
        for lane in range(64):
            assert lib.lh_gemm_f16_piece(p, lane, C.byref(buf)) == 0
            out[p, lane] = tuple(buf)
    return out


def test_arguments_out_of_range_are_refused(lib):
    buf = (C.c_uint32 * 3)()
    assert lib.lh_gemm_f16_piece(40, 0, C.byref(buf)) == -1 and lib.lh_gemm_f16_piece(0, 64, C.byref(buf)) == -1
    assert lib.lh_gemm_f16_piece(0, 0, None) == -1
    for bad in ((8, 0, 0, 0), (0, 32, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
        assert lib.lh_gemm_f16_w_read_off(*bad) == -1


def test_the_forty_pieces_cover_the_stage_exactly_once(lib):
    pc = pieces(lib)
    seen = {}
    for (p, lane), (dst, row, gs) in pc.items():
        assert dst % 16 == 0 and 0 <= dst <= STAGE - 16 and dst not in seen, (p, lane, dst)
        assert dst == p * 1024 + lane * 16                      # what one global -> LDS DMA instruction of 64 lanes x 16 bytes writes
        assert gs < 4 and row < (256 if p >= 24 else 128)
        seen[dst] = (p, lane)
        # the region: X plane p // 8 (rows 16 (p % 8) ..) or W (rows 16 (p - 24) ..), 64-byte rows
        base = W_OFF if p >= 24 else (p // 8) * XP
        assert base + row * 64 <= dst < base + row * 64 + 64, (p, lane)
        assert row == (p - 24 if p >= 24 else p % 8) * 16 + lane // 4
    assert len(seen) == STAGE // 16
    # every (region, row) gets each of its four source granules exactly once
    per_row = {}
    for (p, lane), (dst, row, gs) in pc.items():
        per_row.setdefault((3 if p >= 24 else p // 8, row), []).append(gs)
    assert len(per_row) == 3 * 128 + 256 and all(sorted(v) == [0, 1, 2, 3] for v in per_row.values())
    # eight waves, five pieces each (wave w: w, w + 8, ..): every piece has exactly one owner, the first three of a wave are X and the last two W
    owners = [[w + 8 * pp for pp in range(5)] for w in range(8)]
    assert sorted(sum(owners, [])) == list(range(40))
    assert all([p >= 24 for p in o] == [False, False, False, True, True] for o in owners)


def test_swizzle_is_a_bijection_per_row_group(lib):
    pc = pieces(lib)
    for p in range(40):
        for r4 in range(4):                                   # a piece = four groups of four rows; the rows of a group share the swizzle
            rows = range(4 * r4, 4 * r4 + 4)
            swz = set()
            for r in rows:
                perm = [pc[p, 4 * r + pos][2] for pos in range(4)]     # source granule stored at position pos
                assert sorted(perm) == [0, 1, 2, 3]
                swz.add(tuple(perm))
            assert len(swz) == 1
        # consecutive row groups use different permutations: the four groups of a piece see all four
        assert len({tuple(pc[p, 16 * r4 + pos][2] for pos in range(4)) for r4 in range(4)}) == 4


def test_weight_reads_find_their_granule_and_are_conflict_free(lib):
    pc = pieces(lib)
    where = {dst: (p, row, gs) for (p, lane), (dst, row, gs) in pc.items()}
    for wm in range(8):
        for kk in range(2):
            offs = {}
            for li in range(32):
                for lh in range(2):
                    off = lib.lh_gemm_f16_w_read_off(wm, li, lh, kk)
                    assert off % 16 == 0 and W_OFF <= off <= STAGE - 16
                    p, row, gs = where[off]
                    assert p >= 24 and row == wm * 32 + li and gs == 2 * kk + lh, (wm, li, lh, kk)     # halves 16 kk + 8 lh .. + 7 of the lane's weight row
                    offs[lh * 32 + li] = off
            # ds_read_b128 is served in four groups of 16 lanes - lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same of the upper 32 - and within
            # a group each of the 64 banks (4 bytes, bank (address / 4) % 64) must be touched once.  The X planes, same geometry, are read the same way.
            lower = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
            for g, lanes in enumerate(lower + tuple([l + 32 for l in grp] for grp in lower)):
                banks = []
                for lane in lanes:
                    banks += [(offs[lane] // 4 + e) % 64 for e in range(4)]
                assert len(set(banks)) == 64, (wm, kk, g)


def test_split_and_layout_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_f16_split_main")
    # the runtimes are linked statically: the child then starts whatever its environment preloads, and the environment is passed on as it is
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
           os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "gemm_f16_split_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines() == ["split ok -24", "layout ok"]
