"""not-gpu: the ring image, the column halves and the shape predicate of k_stream_b9w (csrc/stream_b9w_layout.h - the functions the kernel's loader and
MFMA waves and the host's dispatch call), through tests/stream_b9w_layout_main.cpp under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILT = [(maxt, nct) for maxt in (1, 2, 3, 4, 6, 8) for nct in (5, 6, 7, 8)]       # b9w_built: what csrc/stream_b9w.hip instantiates
# (compute units, embd, ff, head size): 7B, 13B, 65B on the 256 units of the target, and on a partition of 64; `small` of tests/weight_probe_ref.py
MODELS = [(256, 4096, 11008, 128), (256, 5120, 13824, 128), (256, 8192, 22016, 128), (64, 4096, 11008, 128), (256, 1024, 2816, 128)]
ADMITTED = [64, 64, 0, 0, 64]                                                       # row counts 65..128 admitted: 65B's w1|w3 needs twelve row tiles


@pytest.fixture(scope="module")
def layout_main(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("b9w") / "stream_b9w_layout_main")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
           os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stream_b9w_layout_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.splitlines()
    return run


def test_every_instantiation_maps_its_image_once_and_fits_the_lds(layout_main):
    assert layout_main("".join(f"i {maxt} {nct}\n" for maxt, nct in BUILT)) == [f"i {maxt} {nct} ok" for maxt, nct in BUILT]
    assert layout_main("i 5 8\ni 6 4\ni 8 9\n") == ["i 5 8 BAD", "i 6 4 BAD", "i 8 9 BAD"]       # not built: the host answers "not applicable"


def test_what_the_predicate_admits_has_an_instantiation(layout_main):
    out = layout_main("".join("s %d %d %d %d\n" % m for m in MODELS))
    assert out == ["s %d %d %d %d ok %d" % (m + (a,)) for m, a in zip(MODELS, ADMITTED)]
