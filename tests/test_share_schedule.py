"""not-gpu: lh_share_schedule, the pure block table a tick derives from the sharing groups of a batch (csrc/share_schedule.h; lh_batch_fork), against
a restatement of the rule.

The rule: groups in ascending order of their lowest member, members ascending, cut into blocks of at most qb rows (2, 4 or 8); chunks = len // 128 full
key chunks lie inside the prefix; a group with chunks == 0 or fewer than min_rows members gets no block, nor does a trailing block of one row;
row_block[j] = the block of row j or 0xFFFFFFFF.  The same corpus runs through tests/share_schedule_main.cpp (the header behind its own main) built
with -fsanitize=address,undefined, as a child process."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_BLOCK = 0xFFFFFFFF
UNSET = 0xDEADBEEF
QBS = (2, 4, 8)
LENS = (0, 127, 128, 129, 383, 384)


class Block(C.Structure):
    _fields_ = [("n", C.c_uint32), ("chunks", C.c_uint32), ("row", C.c_uint32 * 8)]


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    u32p = C.POINTER(C.c_uint32)
    lib.lh_share_schedule.restype = C.c_int
    lib.lh_share_schedule.argtypes = [u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Block), C.c_uint32, u32p]
    return lib


def restated(group, length, qb, min_rows):
    """the rule again, in Python -> ([(chunks, [rows])], row_block)"""
    rows = len(group)
    blocks, rb = [], [NO_BLOCK] * rows
    for g in sorted(set(group)):
        members = [j for j in range(rows) if group[j] == g]
        chunks = length[g] // 128
        if chunks == 0 or len(members) < min_rows:
            continue
        for r in range(0, len(members), qb):
            part = members[r:r + qb]
            if len(part) < 2:
                continue
            for j in part:
                rb[j] = len(blocks)
            blocks.append((chunks, part))
    return blocks, rb


def call(lib, group, length, qb, min_rows, cap, sizing=False, rows=None):
    """one call -> (n, blocks as written [(chunks, rows) or None for an entry left alone], row_block with None for entries left alone)"""
    n_in = len(group)
    g, ln = (C.c_uint32 * max(n_in, 1))(*group), (C.c_uint32 * max(n_in, 1))(*length)
    blocks = (Block * max(cap, 1))()
    for b in blocks:
        b.n = UNSET
    rb = (C.c_uint32 * max(n_in, 1))(*([UNSET] * max(n_in, 1)))
    n = lib.lh_share_schedule(g, ln, n_in if rows is None else rows, qb, min_rows, None if sizing else blocks, cap, rb)
    got = [None if b.n == UNSET else (b.chunks, list(b.row[:b.n])) for b in blocks[:cap]]
    return n, got, [None if x == UNSET else x for x in rb[:n_in]]


def one_group(size, length, rows=64):
    """a group of `size` pods of a batch of `rows`, not neighbours where there is room (every other pod from pod 1 on), the other pods loners"""
    members = list(range(1, 2 * size, 2)) if 2 * size <= rows else list(range(size))
    group, ln = list(range(rows)), [0] * rows
    for j in members:
        group[j], ln[j] = members[0], length
    return group, ln


def corpus():
    """(group, len, qb, min_rows) of the cases: every qb; group sizes 1, 2, qb, qb + 1, 2 qb + 1, 64; every length of LENS; min_rows around the size; interleaved groups"""
    cases = []
    for qb in QBS:
        for size in sorted({1, 2, qb, qb + 1, 2 * qb + 1, 64}):
            for length in LENS:
                for min_rows in sorted({0, 2, max(size - 1, 1), size, size + 1}):
                    cases.append(one_group(size, length) + (qb, min_rows))
        # two groups interleaved over the pod indices, different lengths, and four loners at the end
        for la, lb in ((384, 129), (127, 256), (128, 128)):
            rows = 26
            group, ln = list(range(rows)), [0] * rows
            for j in range(0, 22, 2):
                group[j], ln[j] = 0, la
            for j in range(1, 22, 2):
                group[j], ln[j] = 1, lb
            cases.append((group, ln, qb, 2))
    return cases


def test_schedule_equals_the_restated_rule(lib):
    seen_trailing = seen_none = 0
    for group, ln, qb, min_rows in corpus():
        want_blocks, want_rb = restated(group, ln, qb, min_rows)
        n, got, rb = call(lib, group, ln, qb, min_rows, 0, sizing=True)          # the sizing call: the count and row_block, no block array
        assert n == len(want_blocks) and rb == want_rb, (group, ln, qb, min_rows)
        n2, got, rb = call(lib, group, ln, qb, min_rows, n)                       # the filling call with exactly that capacity
        assert n2 == n and got == want_blocks and rb == want_rb, (group, ln, qb, min_rows, got, want_blocks)
        members = [j for j in range(len(group)) if ln[j]]
        seen_trailing += bool(want_blocks) and len(members) % qb == 1
        seen_none += not want_blocks
        if n:
            assert call(lib, group, ln, qb, min_rows, n - 1) == (-1, [None] * (n - 1), [None] * len(group))   # cap too small: refused, nothing written
            assert call(lib, group, ln, qb, min_rows, n + 3)[1] == want_blocks + [None] * 3                     # room to spare: the rest is left alone
    assert seen_trailing >= 6 and seen_none >= 20


def test_properties_of_the_table(lib):
    """what the tick kernel relies on: every block has 2..qb distinct rows in ascending order, all of one group, row_block is its inverse, chunks >= 1
    and chunks * 128 <= len"""
    for group, ln, qb, min_rows in corpus():
        n, blocks, rb = call(lib, group, ln, qb, min_rows, 32)
        for i, blk in enumerate(blocks[:n]):
            chunks, rows = blk
            assert 2 <= len(rows) <= qb and rows == sorted(set(rows))
            assert len({group[j] for j in rows}) == 1 and 1 <= chunks and chunks * 128 <= ln[rows[0]]
            assert all(rb[j] == i for j in rows)
        assert sum(x != NO_BLOCK for x in rb) == sum(len(b[1]) for b in blocks[:n])


def test_bad_arguments(lib):
    group, ln = one_group(8, 256, rows=16)
    ok = call(lib, group, ln, 4, 2, 8)
    assert ok[0] == 2
    untouched = (-1, [None] * 8, [None] * 16)
    for qb in (0, 1, 3, 5, 16):
        assert call(lib, group, ln, qb, 2, 8) == untouched
    assert call(lib, group, ln, 4, 2, 8, rows=0) == untouched
    assert call(lib, [0] * 65, [128] * 65, 4, 2, 32, rows=65)[0] == -1
    bad = list(group); bad[3] = 5                                   # a group index above the pod: not the group's lowest member
    assert call(lib, bad, ln, 4, 2, 8) == untouched
    bad = list(group); bad[5] = 3                                   # pod 3 is itself a member of group 1: not a lowest member
    assert call(lib, bad, ln, 4, 2, 8) == untouched
    bad = list(ln); bad[5] = 128                                    # members of one group with different lengths
    assert call(lib, group, bad, 4, 2, 8) == untouched
    u32p = C.POINTER(C.c_uint32)
    g = (C.c_uint32 * 16)(*group)
    assert lib.lh_share_schedule(None, g, 16, 4, 2, None, 0, None) == -1
    assert lib.lh_share_schedule(g, C.cast(None, u32p), 16, 4, 2, None, 0, None) == -1
    l16 = (C.c_uint32 * 16)(*ln)
    assert lib.lh_share_schedule(g, l16, 16, 4, 2, None, 0, None) == 2   # row_block is optional


def test_host_shim_mirrors_the_function(built):
    """llamago_ShareSchedule (mlapi.share_schedule) is lh_share_schedule."""
    from llama_go_amd.mlapi import load_product, share_schedule
    ml = load_product()
    for group, ln, qb, min_rows in corpus()[::17]:
        want_blocks, want_rb = restated(group, ln, qb, min_rows)
        assert share_schedule(ml, group, ln, qb, min_rows) == (len(want_blocks), want_blocks, want_rb)
        assert share_schedule(ml, group, ln, qb, min_rows, sizing=True) == (len(want_blocks), [], want_rb)
    assert share_schedule(ml, [0, 0], [128, 128], 3, 2)[0] == -1


def test_corpus_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "share_schedule_main")
    # the runtimes are linked statically: the child then starts whatever its environment preloads, and the environment is passed on as it is
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
           os.path.join(ROOT, "llama.go_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "share_schedule_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower()):
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stderr[-2000:]

    def fmt_blocks(blocks):
        return "".join(f" {c}:{','.join(str(j) for j in rows)}" for c, rows in blocks)

    def fmt_rb(rb):
        return "".join(f" {x}" for x in rb)

    lines, want = [], []
    for group, ln, qb, min_rows in corpus():
        blocks, rb = restated(group, ln, qb, min_rows)
        flat = " ".join(f"{g} {l}" for g, l in zip(group, ln))
        n, rows = len(blocks), len(group)
        lines.append(f"{qb} {min_rows} {n} 0 {rows} {flat}"); want.append(f"{n} |{fmt_blocks(blocks)} |{fmt_rb(rb)}")              # filling, exact capacity
        lines.append(f"{qb} {min_rows} 0 1 {rows} {flat}"); want.append(f"{n} | |{fmt_rb(rb)}")                                      # sizing
        lines.append(f"{qb} {min_rows} {n} 4 {rows} {flat}"); want.append(f"{n} |{fmt_blocks(blocks)} |" + " -" * rows)               # no row_block
        if n:
            lines.append(f"{qb} {min_rows} {n - 1} 0 {rows} {flat}"); want.append("-1 |" + " -" * (n - 1) + " |" + " -" * rows)   # cap too small
    group, ln = one_group(8, 256, rows=16)
    flat = " ".join(f"{g} {l}" for g, l in zip(group, ln))
    for head in ("3 2 8 0 16", "4 2 8 2 16", "4 2 8 3 16"):                                                                          # qb, null group, null len
        lines.append(f"{head} {flat}"); want.append("-1 |" + " -" * 8 + " |" + " -" * 16)
    bad = list(group); bad[3] = 5
    lines.append("4 2 8 0 16 " + " ".join(f"{g} {l}" for g, l in zip(bad, ln))); want.append("-1 |" + " -" * 8 + " |" + " -" * 16)
    lines.append("4 2 4 0 65 " + " ".join("0 128" for _ in range(65))); want.append("-1 |" + " -" * 4 + " |" + " -" * 65)             # rows outside 1..64
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for k, (a, w) in enumerate(zip(got, want)):
        assert a == w, (lines[k][:80], a, w)
