"""Known answers of the reference's own AVX dot product (utils/floats_avx.c `_mm256_dot`, built into oracle/_ref by oracle/Makefile) on
fixed inputs: tests/test_oracle.py pins the checker's lane-order model to them on every machine, also where the reference tree (and so
oracle/_ref) is absent.
    python tests/golden/ref_vdot.py      (after build(), with oracle/_ref/libvdot_avx.so built: writes tests/golden/ref_vdot.json)
The inputs come from an integer hash (no RNG stream, no libm): every numpy builds the same float32 vectors."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (8, 9, 15, 16, 100, 128, 4096, 11008, 11013)


def inputs(n):
    """a, b: float32 [n] in [-2, 2) from a 32-bit integer hash of the index (exact integer arithmetic, one rounding to float32)."""
    out = []
    for salt in (0x9E3779B9, 0x7F4A7C15):
        x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(13)
        x = (x * np.uint64(0x5BD1E995)) & np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(15)
        out.append((x.astype(np.float64) / 2.0 ** 32 * 4.0 - 2.0).astype(np.float32))
    return out


def bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def main():
    lib = C.CDLL(os.path.join(HERE, "..", "..", "oracle", "liboracle.so"))
    if not lib.oracle_has_ref_vdot():
        sys.exit("oracle/_ref/libvdot_avx.so is not built: the answers must come from the reference's own kernel")
    lib.oracle_vdot_ref.restype = None
    lib.oracle_vdot_ref.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float)]
    res = {}
    for n in SIZES:
        a, b = inputs(n)
        r = C.c_float()
        lib.oracle_vdot_ref(a.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(r))
        res[str(n)] = {"value": float(r.value), "float32_bits": bits(r.value)}
    json.dump({"kernel": "utils/floats_avx.c _mm256_dot (oracle/_ref/libvdot_avx.so)", "inputs": "tests/golden/ref_vdot.py inputs(n)", "results": res},
              open(os.path.join(HERE, "ref_vdot.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
