"""not-gpu: lh_feed_schedule, the pure pass schedule lh_batch_feed executes (csrc/feed_schedule.h), against a restatement of the rule.

The rule: a pod with n_tokens >= solo_min is a solo pass (an Eval on its own plan); all other fed rows, in pod order with ascending positions,
are cut into batched passes of at most 64 rows (a pod's rows in one pass are one segment, which may continue in the next pass); a pass of one
row, and the segments of a pass whose row count the `sizes_ok` mask refuses, run solo; a query block is at most qb consecutive rows of ONE
segment of a batched pass."""
import ctypes as C

import numpy as np
import pytest

BATCHED, SOLO = 0, 1
ALL_SIZES = (1 << 64) - 1


class Pass(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("kind", "seg0", "nseg", "blk0", "nblk", "rows")]


class Seg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("pod", "row0", "n", "pos0")]


class Block(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("row0", "n")]


@pytest.fixture(scope="module")
def lib(built):
    import llama_go_amd as pkg
    lib = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    u32p = C.POINTER(C.c_uint32)
    lib.lh_feed_schedule.restype = C.c_int
    lib.lh_feed_schedule.argtypes = [u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(Pass), C.c_uint32, C.POINTER(Seg), C.c_uint32,
                                     C.POINTER(Block), C.c_uint32, u32p]
    return lib


def schedule(lib, n_tokens, past, solo_min=129, qb=8, sizes_ok=ALL_SIZES):
    """[(kind, [(pod, row0, n, pos0)], [(row0, n)])] per pass, through the sizing call and the filling call"""
    rows = len(n_tokens)
    nt, ps = (C.c_uint32 * rows)(*n_tokens), (C.c_uint32 * rows)(*past)
    counts = (C.c_uint32 * 3)()
    n = lib.lh_feed_schedule(nt, ps, rows, solo_min, qb, sizes_ok, None, 0, None, 0, None, 0, counts)
    assert n == counts[0]
    passes, segs, blocks = (Pass * max(counts[0], 1))(), (Seg * max(counts[1], 1))(), (Block * max(counts[2], 1))()
    assert lib.lh_feed_schedule(nt, ps, rows, solo_min, qb, sizes_ok, passes, counts[0], segs, counts[1], blocks, counts[2], counts) == n
    out = []
    for p in passes[:n]:
        out.append((p.kind, [(s.pod, s.row0, s.n, s.pos0) for s in segs[p.seg0:p.seg0 + p.nseg]], [(b.row0, b.n) for b in blocks[p.blk0:p.blk0 + p.nblk]], p.rows))
    return out


def restated(n_tokens, past, solo_min, qb, sizes_ok):
    """the rule again, in Python"""
    flat = [(i, past[i] + j) for i, n in enumerate(n_tokens) if 0 < n < solo_min for j in range(n)]
    out = []
    for c in range(0, len(flat), 64):
        rows, segs = flat[c:c + 64], []
        for r, (pod, pos) in enumerate(rows):
            if segs and segs[-1][0] == pod:
                segs[-1][2] += 1
            else:
                segs.append([pod, r, 1, pos])
        if len(rows) >= 2 and (sizes_ok >> (len(rows) - 1)) & 1:
            out.append((BATCHED, [tuple(s) for s in segs], [(s[1] + r, min(qb, s[2] - r)) for s in segs for r in range(0, s[2], qb)], len(rows)))
        else:
            out += [(SOLO, [(s[0], 0, s[2], s[3])], [], s[2]) for s in segs]
    return out + [(SOLO, [(i, 0, n, past[i])], [], n) for i, n in enumerate(n_tokens) if n >= solo_min]


def check_properties(n_tokens, past, solo_min, qb, sched):
    seen = {}
    order = {}
    for kind, segs, blocks, rows in sched:
        assert rows == sum(s[2] for s in segs)
        if kind == BATCHED:
            assert 2 <= rows <= 64
            assert [s[1] for s in segs] == list(np.cumsum([0] + [s[2] for s in segs[:-1]])), "segments tile the pass in order"
            assert [s[0] for s in segs] == sorted(set(s[0] for s in segs)), "pod order, one segment per pod and pass"
            covered = []
            for row0, n in blocks:
                assert 1 <= n <= qb
                inside = [s for s in segs if s[1] <= row0 and row0 + n <= s[1] + s[2]]
                assert len(inside) == 1, "a block never spans segments"
                covered += list(range(row0, row0 + n))
            assert covered == list(range(rows)), "blocks cover every row of a batched pass once, in order"
        else:
            assert len(segs) == 1 and segs[0][1] == 0 and not blocks
        for pod, row0, n, pos0 in segs:
            assert n >= 1
            for j in range(n):
                assert (pod, pos0 + j) not in seen, "a fed row appears exactly once"
                seen[(pod, pos0 + j)] = kind
            assert order.get(pod, past[pod]) == pos0, "a pod's rows come in ascending positions, without gaps"
            order[pod] = pos0 + n
    assert set(seen) == {(i, past[i] + j) for i, n in enumerate(n_tokens) for j in range(n)}
    for i, n in enumerate(n_tokens):
        if n >= solo_min:
            assert all(seen[(i, past[i] + j)] == SOLO for j in range(n))


def test_random_inputs_follow_the_rule(lib):
    rng = np.random.default_rng(7)
    for it in range(3000):
        rows = int(rng.integers(1, 65))
        solo_min = int(rng.choice([1, 2, 5, 17, 65, 129, 1000]))
        qb = int(rng.choice([1, 2, 4, 8]))
        hi = int(rng.choice([2, 4, 9, 70, 140]))
        n_tokens = [int(x) * int(rng.random() < 0.7) for x in rng.integers(0, hi, rows)]
        past = [int(x) for x in rng.integers(0, 500, rows)]
        sizes_ok = ALL_SIZES if it % 3 else int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))
        got = schedule(lib, n_tokens, past, solo_min, qb, sizes_ok)
        assert got == restated(n_tokens, past, solo_min, qb, sizes_ok), (n_tokens, past, solo_min, qb, hex(sizes_ok))
        check_properties(n_tokens, past, solo_min, qb, got)
        if it % 50 == 0:
            assert got == schedule(lib, n_tokens, past, solo_min, qb, sizes_ok), "deterministic"


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 128, 129])
def test_totals_around_the_pass_size(lib, total):
    """`total` rows over pods of at most 7 tokens: ceil(total / 64) passes, a one-row remainder as that pod's own Eval"""
    n_tokens, left = [], total
    while left:
        n_tokens.append(min(left, 1 + len(n_tokens) % 7))
        left -= n_tokens[-1]
    assert len(n_tokens) <= 64
    past = [3 * i for i in range(len(n_tokens))]
    got = schedule(lib, n_tokens, past)
    assert got == restated(n_tokens, past, 129, 8, ALL_SIZES)
    check_properties(n_tokens, past, 129, 8, got)
    assert [p[3] for p in got] == [64] * (total // 64) + ([total % 64] if total % 64 else [])
    assert [p[0] for p in got] == [BATCHED] * (total // 64) + ([BATCHED if total % 64 > 1 else SOLO] if total % 64 else [])


def test_one_pod_over_several_passes(lib):
    got = schedule(lib, [3, 128, 2], [0, 10, 7])
    assert [(k, segs) for k, segs, _, _ in got] == [
        (BATCHED, [(0, 0, 3, 0), (1, 3, 61, 10)]),
        (BATCHED, [(1, 0, 64, 71)]),
        (BATCHED, [(1, 0, 3, 135), (2, 3, 2, 7)])]
    assert got[0][2][:2] == [(0, 3), (3, 8)] and got[0][2][-1] == (59, 5)      # blocks restart at the segment and end with it
    check_properties([3, 128, 2], [0, 10, 7], 129, 8, got)


def test_solo_threshold(lib):
    for n, kinds in ((128, [BATCHED, BATCHED, BATCHED]), (129, [BATCHED, SOLO])):
        got = schedule(lib, [2, n, 2], [0, 0, 0], solo_min=129)
        assert [p[0] for p in got] == kinds, n
        check_properties([2, n, 2], [0, 0, 0], 129, 8, got)
    got = schedule(lib, [2, 129, 2], [0, 5, 0])
    assert got[0] == (BATCHED, [(0, 0, 2, 0), (2, 2, 2, 0)], [(0, 2), (2, 2)], 4) and got[1] == (SOLO, [(1, 0, 129, 5)], [], 129)


def test_refused_pass_sizes_run_their_segments_solo(lib):
    """sizes_ok without bit 2: a pass of three rows is refused (plan_batch_rows_ok), its segments are Evals of their own; no size allowed: all solo"""
    assert [p[0] for p in schedule(lib, [1, 2], [4, 0], sizes_ok=ALL_SIZES & ~(1 << 2))] == [SOLO, SOLO]
    assert [p[0] for p in schedule(lib, [1, 2], [4, 0])] == [BATCHED]
    got = schedule(lib, [5, 0, 70], [0, 0, 1], sizes_ok=0)
    assert got == [(SOLO, [(0, 0, 5, 0)], [], 5), (SOLO, [(2, 0, 59, 1)], [], 59), (SOLO, [(2, 0, 11, 60)], [], 11)]


def test_all_zero_and_bad_arguments(lib):
    assert schedule(lib, [0, 0, 0], [1, 2, 3]) == []
    nt = (C.c_uint32 * 2)(1, 1)
    assert lib.lh_feed_schedule(nt, nt, 0, 129, 8, ALL_SIZES, None, 0, None, 0, None, 0, None) == -1
    assert lib.lh_feed_schedule(nt, nt, 65, 129, 8, ALL_SIZES, None, 0, None, 0, None, 0, None) == -1
    assert lib.lh_feed_schedule(nt, nt, 2, 129, 0, ALL_SIZES, None, 0, None, 0, None, 0, None) == -1
    assert lib.lh_feed_schedule(None, nt, 2, 129, 8, ALL_SIZES, None, 0, None, 0, None, 0, None) == -1


def test_the_feed_entry_points_are_declared_and_exported(built):
    import os
    import llama_go_amd as pkg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    go = C.CDLL(pkg.LIBLLAMAGO)
    assert hasattr(hip, "lh_batch_feed") and hasattr(hip, "lh_feed_schedule") and hasattr(go, "llamago_BatchFeed")
    assert "lh_batch_feed(" in open(os.path.join(root, "include", "llamahip.h")).read()
    assert "llamago_BatchFeed(" in open(os.path.join(root, "include", "llamago_ext.h")).read()
    assert "C.lh_batch_feed(" in open(os.path.join(root, "llama.go_amd", "go", "ml_hip_pods.go")).read()
