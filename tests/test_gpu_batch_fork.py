"""-m gpu: lh_batch_fork - a pod's evaluated prompt prefix for other pods of the batch - and the ticks that read a shared prefix once per block of
member rows (k_attention_split_shared, csrc/kernels_attn_share.h).

The shared tick kernel performs, per query row, the operations of k_attention_split in their order, so the feature is tested by EQUALITY, with no
tolerance: LLAMAHIP_SHARE_ROW_ATTN=1 keeps the per-row kernels in-process and is the reference.
 1. the copy: rows [0, n_pos) of every layer, K and V, byte for byte; nothing beyond; nobody else's cache;
 2. ticks byte-equal to the per-row kernels (ids of every tick, the last logits), the route trace proves which kernel ran; QB = 8 / 4 / 2; a sampling batch;
 3. shared lengths 127 / 128 / 129: no full chunk, exactly one;
 4. a fork equals evaluating the prefix oneself (caches, ids, fp32 logits byte-equal);
 5. every writer below the shared length makes the pod leave its group; joining and re-forming;
 6. every refusal leaves the batch as it was; a window of 256 (no split partials): the fork copies, the ticks run the single-pass kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_batch import make_prompts   # noqa: E402
from test_gpu_batch_feed import HD128   # noqa: E402
from llama_go_amd.mlapi import Batch, MLError, make_hparams, route_trace, share_schedule   # noqa: E402

pytestmark = pytest.mark.gpu

V, D, LAYERS = HD128["vocab"], HD128["embd"], HD128["layers"]
SEED = 8


def model(product, ctx, int8):
    m = product.NewSyntheticModel(make_hparams(**HD128, ctx=ctx), SEED)
    if int8:
        m.QuantizeQ8()
    return m


def shared_entries(trace):
    return [e for e in trace if e.startswith("k_attention_split_shared/")]


def row_entries(trace):
    return [e for e in trace if e.startswith(("k_attention_split/rows", "k_attention/rows"))]


def table_entries(trace):
    return [e for e in trace if e.startswith("share_table/")]


def set_switches(monkeypatch, row_attn, qb=None, min_rows=None):
    monkeypatch.setenv("LLAMAHIP_SHARE_ROW_ATTN", "1" if row_attn else "0")
    for name, v in (("LLAMAHIP_SHARE_QB", qb), ("LLAMAHIP_SHARE_MIN", min_rows)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def cache_rows(b, pod, ctx, lo, hi):
    """K and V rows [lo, hi) of every layer slot of pod's cache: [2][layers][hi - lo][embd]"""
    return np.stack([np.stack([b.CacheRead(pod, which, (l * ctx + lo) * D, (hi - lo) * D).reshape(hi - lo, D) for l in range(LAYERS)]) for which in (0, 1)])


# ---- 1. the copy -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True])
def test_fork_copies_the_prefix_and_nothing_else(product, int8):
    ctx, n_pos = 384, 150
    m = model(product, ctx, int8)
    b = Batch(m, ctx, 6)
    try:
        rng = np.random.default_rng(1)
        sentinel = {p: rng.standard_normal((2, LAYERS * ctx * D)).astype(np.float32) for p in (2, 5)}
        for p in (2, 5):
            for which in (0, 1):
                b.CacheWrite(p, which, 0, sentinel[p][which])
        prompt = make_prompts(rng, V, [200])[0]
        b.Feed([prompt, [1], [2], [3], [4], [5]], [0] * 6)        # (pods 2 and 5 write their own row 0: inside the range the fork overwrites)
        pod1 = cache_rows(b, 1, ctx, 0, ctx)
        assert b.ShareInfo() == ([0, 1, 2, 3, 4, 5], [0] * 6)
        b.Fork(0, [5, 2], n_pos)
        src = cache_rows(b, 0, ctx, 0, n_pos)
        assert np.all(np.isfinite(src)) and np.abs(src).max() > 0
        for p in (2, 5):
            assert cache_rows(b, p, ctx, 0, n_pos).tobytes() == src.tobytes(), f"pod {p}: rows [0, {n_pos}) differ from the source's"
            want = sentinel[p].reshape(2, LAYERS, ctx, D)[:, :, n_pos:]
            assert cache_rows(b, p, ctx, n_pos, ctx).tobytes() == want.tobytes(), f"pod {p}: a sentinel at a position >= {n_pos} was overwritten"
        assert cache_rows(b, 1, ctx, 0, ctx).tobytes() == pod1.tobytes()
        assert b.ShareInfo() == ([0, 1, 0, 3, 4, 0], [n_pos, 0, n_pos, 0, 0, n_pos])
    finally:
        b.free()
        m.free()


# ---- 2. ticks are bit-identical, and the shared kernel really ran ------------------------------------------------------------------------------------
TICK_CTX, TICK_PODS = 640, 12
GROUP_A, LEN_A = [0, 2, 3, 5, 6, 8, 9, 10, 11], 300      # nine pods that are not neighbours: two full chunks and a partial one inside the prefix
GROUP_B, LEN_B = [1, 7], 128
LONER = 4
SUFFIX = {2: 1, 3: 2, 5: 3, 6: 4, 8: 5, 9: 6, 10: 7, 11: 1, 7: 3}    # fed behind the fork; pods 0 and 1 are NOT fed: they stand at len, their ticks see len + 1 keys
# 70 ticks leave the members (at 300..307) below 384; a second leg of 150 takes every member across the chunk boundaries at 384 and 512
TICK_LEGS = (70, 150)
BLOCKS = {8: 2, 4: 3, 2: 5}                                              # 8 + (1) | 2;  4 + 4 + (1) | 2;  2 + 2 + 2 + 2 + (1) | 2


def run_shared_ticks(m, monkeypatch, qb, row_attn, sampling):
    set_switches(monkeypatch, row_attn, qb)
    rng = np.random.default_rng(77)
    pre_a, pre_b, lone = make_prompts(rng, V, [LEN_A, LEN_B, 40])
    suffix = {p: make_prompts(rng, V, [n])[0] for p, n in SUFFIX.items()}
    b = Batch(m, TICK_CTX, TICK_PODS)
    try:
        assert b.batched
        first = [[9]] * TICK_PODS
        first[0], first[1], first[LONER] = pre_a, pre_b, lone
        pos = [len(t) for t in first]
        if sampling:
            b.SetSampler(seed=5, ringSize=64)
            feed = lambda toks, past: b.FeedSample(toks, past)   # noqa: E731
        else:
            feed = lambda toks, past: b.Feed(toks, past)         # noqa: E731
        pending = feed(first, [0] * TICK_PODS)
        b.Fork(0, GROUP_A[1:], LEN_A)
        b.Fork(1, GROUP_B[1:], LEN_B)
        toks = [suffix.get(p, []) for p in range(TICK_PODS)]
        past = [LEN_A if p in GROUP_A else LEN_B if p in GROUP_B else 0 for p in range(TICK_PODS)]
        for p, t in enumerate(feed(toks, past)):
            if t is not None:
                pending[p], pos[p] = t, past[p] + len(toks[p])
        group, length = b.ShareInfo()
        assert [group[p] for p in GROUP_A] == [0] * 9 and [length[p] for p in GROUP_A] == [LEN_A] * 9
        assert [group[p] for p in GROUP_B] == [1, 1] and [length[p] for p in GROUP_B] == [LEN_B] * 2 and (group[LONER], length[LONER]) == (LONER, 0)
        out = []

        def ticks(n):
            nonlocal pending, pos
            if sampling:
                ids = [[] for _ in range(TICK_PODS)]
                for _ in range(n):
                    for p, t in enumerate(b.Tick()):
                        ids[p].append(t)
                lg = None
            else:
                ids, lg = b.Decode(pending, pos, n, want_logits=True)
            pending, pos = [s[-1] for s in ids], [x + n for x in pos]
            return ids, lg

        for n in TICK_LEGS:
            (ids, lg), tr = route_trace(lambda: ticks(n))
            out.append((ids, lg, tr))
        return out
    finally:
        b.free()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("sampling", [False, True])
@pytest.mark.parametrize("qb", [8, 4, 2])
def test_shared_ticks_are_bit_identical_to_the_per_row_kernels(product, monkeypatch, qb, sampling, int8):
    m = model(product, TICK_CTX, int8)
    try:
        shared = run_shared_ticks(m, monkeypatch, qb, False, sampling)
        rows = run_shared_ticks(m, monkeypatch, qb, True, sampling)
    finally:
        m.free()
    nch = (TICK_CTX + 127) // 128
    for leg, ((ids_s, lg_s, tr_s), (ids_r, lg_r, tr_r)) in enumerate(zip(shared, rows)):
        assert ids_s == ids_r, f"leg {leg}: ids differ between the shared and the per-row kernels"
        if not sampling:
            assert np.all(np.isfinite(lg_s))
            assert lg_s.tobytes() == lg_r.tobytes(), f"leg {leg}: {np.count_nonzero(lg_s != lg_r)} logits of the last tick differ"
        assert not row_entries(tr_s) and not shared_entries(tr_r) and not table_entries(tr_r), (tr_s, tr_r)
        if leg == 0:   # (the first tick runs eagerly, the second is captured; the ticks behind them replay the graph and enqueue nothing)
            want = f"k_attention_split_shared/c{nch}/qb{qb}/b{BLOCKS[qb]}/n{len(GROUP_A) - 1 + len(GROUP_B)}"
            assert shared_entries(tr_s) and set(shared_entries(tr_s)) == {want}, tr_s
            assert row_entries(tr_r) and all(e.startswith(f"k_attention_split/rows/c{nch}/") for e in row_entries(tr_r)), tr_r
    assert table_entries(shared[0][2]) == [f"share_table/b{BLOCKS[qb]}"] and not table_entries(shared[1][2])   # sent once: nothing changed afterwards


# ---- 3. short prefixes ---------------------------------------------------------------------------------------------------------------------------
def run_short(m, monkeypatch, n_pos, row_attn):
    set_switches(monkeypatch, row_attn)
    ctx = 384
    rng = np.random.default_rng(n_pos)
    prompt, s1, s2 = make_prompts(rng, V, [140, 2, 3])
    b = Batch(m, ctx, 4)
    try:
        pending = b.Feed([prompt, [1], [2], [3]], [0] * 4)
        b.Fork(0, [1, 2], n_pos)
        got = b.Feed([[], s1, s2, []], [0, n_pos, n_pos, 0])
        pending[1], pending[2] = got[1], got[2]
        info = b.ShareInfo()
        (ids, lg), tr = route_trace(lambda: b.Decode(pending, [140, n_pos + 2, n_pos + 3, 1], 12, want_logits=True))
        return ids, lg, tr, info
    finally:
        b.free()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("n_pos", [127, 128, 129])
def test_short_prefixes(product, monkeypatch, n_pos, int8):
    m = model(product, 384, int8)
    try:
        ids_s, lg_s, tr_s, info = run_short(m, monkeypatch, n_pos, False)
        ids_r, lg_r, tr_r, _ = run_short(m, monkeypatch, n_pos, True)
    finally:
        m.free()
    assert info == ([0, 0, 0, 3], [n_pos] * 3 + [0])
    n, blocks, row_block = share_schedule(product, info[0], info[1], 4, 2)
    assert ids_s == ids_r and lg_s.tobytes() == lg_r.tobytes()
    assert row_entries(tr_r) and not shared_entries(tr_r)
    if n_pos < 128:
        assert n == 0 and not shared_entries(tr_s) and row_entries(tr_s) and not table_entries(tr_s), tr_s
    else:
        assert (n, blocks) == (1, [(1, [0, 1, 2])])                  # exactly one chunk is shared
        assert set(shared_entries(tr_s)) == {"k_attention_split_shared/c3/qb4/b1/n3"} and not row_entries(tr_s), tr_s


# ---- 4. fork equals evaluating the prefix oneself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True])
def test_fork_equals_evaluating_the_prefix_oneself(product, monkeypatch, int8):
    set_switches(monkeypatch, False)
    ctx, n_pre, n_ticks = 384, 200, 20
    rng = np.random.default_rng(4)
    prefix, s0, s1, s2 = make_prompts(rng, V, [n_pre, 2, 5, 1])
    m = model(product, ctx, int8)
    res = {}
    try:
        for forked in (False, True):
            b = Batch(m, ctx, 3)
            b.Feed([prefix, [1], [2]], [0, 0, 0])
            if forked:
                b.Fork(0, [1, 2], n_pre)
            else:
                b.Feed([[], prefix, []], [0, 0, 0])              # each pod its prefix in a call of its own
                b.Feed([[], [], prefix], [0, 0, 0])
                pre = [cache_rows(b, p, ctx, 0, n_pre) for p in range(3)]
                # the precondition (the parent's determinism): the same prompt evaluated on three pods leaves byte-equal caches
                assert pre[1].tobytes() == pre[2].tobytes() and pre[0].tobytes() == pre[1].tobytes()
            pending = b.Feed([s0, s1, s2], [n_pre] * 3)
            pos = [n_pre + len(s) for s in (s0, s1, s2)]
            (ids, lg), tr = route_trace(lambda: b.Decode(pending, pos, n_ticks, want_logits=True))
            res[forked] = (pending, ids, lg, [cache_rows(b, p, ctx, 0, pos[p] + n_ticks) for p in range(3)], tr)
            b.free()
    finally:
        m.free()
    own, fork = res[False], res[True]
    assert shared_entries(fork[4]) and not shared_entries(own[4])
    assert fork[0] == own[0] and fork[1] == own[1]
    for p in range(3):
        assert fork[3][p].tobytes() == own[3][p].tobytes(), f"pod {p}: the caches differ"
    print(f"int8 {int8}: {np.count_nonzero(fork[2] != own[2])} last logits differ between the fork and the pods' own evaluation")
    assert fork[2].tobytes() == own[2].tobytes()


# ---- 5. leaving a group --------------------------------------------------------------------------------------------------------------------------
LEAVE_CTX, LEAVE_LEN = 384, 150


def leave_setup(m, keep=None):
    """five pods: 0..3 share [0, 150) (pod 0 evaluated 200 tokens), pod 4 is a loner; pods 1..3 stand behind suffixes of 2 tokens"""
    rng = np.random.default_rng(5)
    prompt, lone = make_prompts(rng, V, [200, 30])
    sfx = make_prompts(rng, V, [2, 2, 2])
    b = Batch(m, LEAVE_CTX, 5)
    if keep is not None:
        b.SetKeepCount(keep)
    pending = b.Feed([prompt, [1], [2], [3], lone], [0] * 5)
    b.Fork(0, [1, 2, 3], LEAVE_LEN)
    got = b.Feed([[], sfx[0], sfx[1], sfx[2], []], [0, LEAVE_LEN, LEAVE_LEN, LEAVE_LEN, 0])
    pending[1:4] = got[1:4]
    assert b.ShareInfo() == ([0, 0, 0, 0, 4], [LEAVE_LEN] * 4 + [0])
    return b, pending, [200, LEAVE_LEN + 2, LEAVE_LEN + 2, LEAVE_LEN + 2, 30]


def w_feed(b, st):
    st["pending"][2] = b.Feed([[], [], [7, 8, 9], [], []], [0, 0, 100, 0, 0])[2]
    st["pos"][2] = 103
    return [0, 0, 2, 0, 4], [LEAVE_LEN, LEAVE_LEN, 0, LEAVE_LEN, 0]


def w_prompt(b, st):
    prompts = [[3, 1, 4, 1, 5], [9, 2], [6, 5, 3], [5], [8, 9, 7, 9]]
    st["pending"], st["pos"] = b.Prompt(prompts), [len(p) for p in prompts]
    return [0, 1, 2, 3, 4], [0] * 5


def w_set(b, st):
    st["pos"][1] = 100
    b.Set(st["pending"], st["pos"])
    return [0, 1, 0, 0, 4], [LEAVE_LEN, 0, LEAVE_LEN, LEAVE_LEN, 0]


def w_cache_write(b, st):
    b.CacheWrite(3, 1, (1 * LEAVE_CTX + 10) * D, np.full(3 * D, 0.25, dtype=np.float32))   # V rows 10..12 of layer slot 1
    return [0, 0, 0, 3, 4], [LEAVE_LEN, LEAVE_LEN, LEAVE_LEN, 0, 0]


WRITERS = {"feed": w_feed, "prompt": w_prompt, "set": w_set, "cache_write": w_cache_write}


def run_writer(m, monkeypatch, name, row_attn):
    set_switches(monkeypatch, row_attn)
    b, pending, pos = leave_setup(m)
    try:
        st = dict(pending=pending, pos=pos)
        before = b.Decode(st["pending"], st["pos"], 3)
        st["pending"], st["pos"] = [s[-1] for s in before], [x + 3 for x in st["pos"]]
        want_info = WRITERS[name](b, st)
        info = b.ShareInfo()
        if name == "set":                                      # (Set placed the pods: the ticks go on from there)
            ids, tr = route_trace(lambda: [b.Tick() for _ in range(6)])
            ids = [list(x) for x in zip(*ids)]
        else:
            ids, tr = route_trace(lambda: b.Decode(st["pending"], st["pos"], 6))
        return before, ids, tr, info, want_info, b.ShareInfo()
    finally:
        b.free()


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_a_writer_below_the_shared_length_makes_the_pod_leave(product, monkeypatch, name):
    m = model(product, LEAVE_CTX, False)
    try:
        before_s, ids_s, tr_s, info, want_info, info_after = run_writer(m, monkeypatch, name, False)
        before_r, ids_r, tr_r, _, _, _ = run_writer(m, monkeypatch, name, True)
    finally:
        m.free()
    assert info == tuple(want_info) and info_after == tuple(want_info)
    assert before_s == before_r and ids_s == ids_r
    assert len(table_entries(tr_s)) == 1, tr_s                         # the table changed: the next tick re-sent it, once
    if name == "prompt":
        assert table_entries(tr_s) == ["share_table/b0"] and not shared_entries(tr_s) and row_entries(tr_s)
    else:
        assert table_entries(tr_s) == ["share_table/b1"], tr_s        # three members left: one block of three (QB = 4)
    assert not table_entries(tr_r) and not shared_entries(tr_r)


def run_swap(m, monkeypatch, row_attn):
    set_switches(monkeypatch, row_attn)
    b, pending, pos = leave_setup(m, keep=0)
    try:
        out = []
        for n in (190, 50):                                    # pod 0 (at 200) reaches the window's end after 184 ticks, pods 1..3 (at 152) after 232
            ticks = [route_trace(b.Tick) for _ in range(n)]
            out.append(([t[0] for t in ticks], b.ShareInfo(), {k: table_entries(t[1]) for k, t in enumerate(ticks) if table_entries(t[1])}))
        return out
    finally:
        b.free()


def test_a_context_swap_makes_the_pod_leave(product, monkeypatch):
    """KeepCount 0: at the window's end a pod re-feeds half its window at position 0 on its own plan - below the shared length.  The swap needs the
    tokens of the forked prefix, which the destinations know only through the fork's history copy."""
    m = model(product, LEAVE_CTX, False)
    try:
        shared = run_swap(m, monkeypatch, False)
        rows = run_swap(m, monkeypatch, True)
    finally:
        m.free()
    assert [s[0] for s in shared] == [r[0] for r in rows]
    assert shared[0][1] == ([0, 1, 1, 1, 4], [0, LEAVE_LEN, LEAVE_LEN, LEAVE_LEN, 0])      # pod 0 swapped and left; the others still share
    assert shared[1][1] == ([0, 1, 2, 3, 4], [0] * 5)                                         # pods 1..3 swapped on one tick: nothing is left to share
    # the table is re-sent by the tick that swaps (the re-fed Eval notes itself on the pod's plan, the batch looks before it enqueues the tick):
    # tick 0 the block of four, tick 184 (pod 0 at 200 + 184 = the window's end) the block of three, tick 232 = 190 + 42 (pods 1..3) no block
    assert shared[0][2] == {0: ["share_table/b1"], 184: ["share_table/b1"]}, shared[0][2]
    assert shared[1][2] == {42: ["share_table/b0"]}, shared[1][2]
    assert not rows[0][2] and not rows[1][2]


def run_fork_behind_ticks(m, forked):
    """pod 0 evaluates the 150-token prefix, BOTH pods tick 20 times (the host has not read those ticks' tokens into the histories yet), then pod 1
    gets the prefix - by the fork, or by evaluating it itself - and its suffix, and runs through the window's end (KeepCount 0)"""
    rng = np.random.default_rng(9)
    prefix, sfx = make_prompts(rng, V, [LEAVE_LEN, 2])
    b = Batch(m, LEAVE_CTX, 2)
    try:
        b.SetKeepCount(0)
        b.Feed([prefix, [1]], [0, 0])
        before = [b.Tick() for _ in range(20)]                 # pod 1 evaluates tokens at positions 1..20: inside the range the fork overwrites
        if forked:
            b.Fork(0, [1], LEAVE_LEN)
        else:
            b.Feed([[], prefix], [0, 0])
        fed = b.Feed([[], sfx], [0, LEAVE_LEN])[1]
        ids = [b.Tick() for _ in range(250)]                   # pod 1 (at 152) swaps on tick 232 and re-feeds tokens 0..191 of ITS history
        return before, fed, ids, b.ShareInfo()
    finally:
        b.free()


def test_fork_behind_ticks_leaves_a_history_a_context_swap_can_use(product, monkeypatch):
    """Ticks are recorded in the pods' token histories only when the host next reads the ids.  A fork behind such ticks must not let the
    destination's old tokens land, later, on the history it copied: the swap at the window's end re-feeds that history, and the ids behind it must be
    those of a pod that evaluated the prefix itself (same Eval, byte-equal cache: the precondition of the fork-equals-own-evaluation test)."""
    set_switches(monkeypatch, False)
    m = model(product, LEAVE_CTX, False)
    try:
        fork = run_fork_behind_ticks(m, True)
        own = run_fork_behind_ticks(m, False)
    finally:
        m.free()
    assert fork[0] == own[0] and fork[1] == own[1]
    assert fork[2][:232] == own[2][:232]
    assert fork[2] == own[2], "the ids behind pod 1's context swap differ: its history does not name the tokens its cache holds"
    assert fork[3] == own[3] == ([0, 1], [0, 0])                  # (pod 0, at 170, swapped on tick 214: the pair dissolved)


def test_groups_dissolve_join_and_re_form(product, monkeypatch):
    set_switches(monkeypatch, False)
    m = model(product, LEAVE_CTX, False)
    b, pending, pos = leave_setup(m)
    try:
        b.Fork(1, [4], LEAVE_LEN)                              # pod 1 stands in a group of exactly that length: pod 4 joins it
        assert b.ShareInfo() == ([0, 0, 0, 0, 0], [LEAVE_LEN] * 5)
        b.Fork(2, [3], 120)                                    # another length: pods 2 and 3 leave and form a group of their own
        assert b.ShareInfo() == ([0, 0, 2, 2, 0], [LEAVE_LEN, LEAVE_LEN, 120, 120, LEAVE_LEN])
        b.Feed([[], [], [], [5], []], [0, 0, 0, 60, 0])        # pod 3 leaves: a group of one dissolves
        assert b.ShareInfo() == ([0, 0, 2, 3, 0], [LEAVE_LEN, LEAVE_LEN, 0, 0, LEAVE_LEN])
        b.Fork(0, [2], 100)                                    # the source re-forms at another length: pods 1 and 4 stay a group
        assert b.ShareInfo() == ([0, 1, 0, 3, 1], [100, LEAVE_LEN, 100, 0, LEAVE_LEN])
    finally:
        b.free()
        m.free()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refused_forks_leave_the_batch_as_it_was(product, monkeypatch):
    set_switches(monkeypatch, False)
    m = model(product, LEAVE_CTX, False)
    try:
        b, pending, pos = leave_setup(m)
        want = b.Decode(pending, pos, 4)
        b.free()
        b, pending, pos = leave_setup(m)
        info = b.ShareInfo()
        caches = [cache_rows(b, p, LEAVE_CTX, 0, 210) for p in range(5)]
        bad = [((5, [1], 10), "outside the batch"), ((0, [1, 5], 10), "outside the batch"), ((0, [1, 0], 10), "source or named twice"),
               ((0, [1, 2, 1], 10), "source or named twice"), ((0, [], 10), "no destination"), ((0, [1], 0), "no position"),
               ((0, [1], 201), "stands at 200"), ((4, [1], 31), "stands at 30")]
        for args, msg in bad:
            with pytest.raises(MLError, match=msg):
                b.Fork(*args)
        assert b.ShareInfo() == info
        for p in range(5):
            assert cache_rows(b, p, LEAVE_CTX, 0, 210).tobytes() == caches[p].tobytes()
        assert b.Decode(pending, pos, 4) == want
        b.free()
        fresh = Batch(m, LEAVE_CTX, 2)
        with pytest.raises(MLError, match="not placed yet"):
            fresh.Fork(0, [1], 1)                              # the host mirror has no positions yet
        fresh.free()
    finally:
        m.free()


def test_a_window_without_split_partials_forks_and_ticks_as_before(product, monkeypatch):
    """ctx 256: the plan has no split partials, so there is nothing for the ticks to share - the fork copies, the group is recorded, the ticks run
    k_attention on the row table."""
    set_switches(monkeypatch, False)
    ctx, n_pos = 256, 140
    m = model(product, ctx, False)
    b = Batch(m, ctx, 3)
    try:
        prompt = make_prompts(np.random.default_rng(6), V, [160])[0]
        pending = b.Feed([prompt, [1], [2]], [0, 0, 0])
        b.Fork(0, [1, 2], n_pos)
        assert cache_rows(b, 1, ctx, 0, n_pos).tobytes() == cache_rows(b, 0, ctx, 0, n_pos).tobytes()
        got = b.Feed([[], [4, 5], [6]], [0, n_pos, n_pos])
        pending[1:] = got[1:]
        assert b.ShareInfo() == ([0, 0, 0], [n_pos] * 3)
        ids, tr = route_trace(lambda: b.Decode(pending, [160, n_pos + 2, n_pos + 1], 5))
        assert row_entries(tr) and all(e.startswith("k_attention/rows/") for e in row_entries(tr)) and not shared_entries(tr) and not table_entries(tr), tr
        assert b.ShareInfo() == ([0, 0, 0], [n_pos] * 3)
    finally:
        b.free()
        m.free()


def test_fork_refuses_a_batch_of_layer_shard_stages(product):
    """A batch of layer-shard stages, built through the C-ABI as tests/test_gpu_batch_feed.py builds it (the host mirror only builds whole-model batches):
    LH_EUNSUPPORTED before anything is enqueued, the group state untouched."""
    import ctypes as C
    import llama_go_amd as pkg
    lh = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    VP, u32p, u64 = C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64

    class Layer(C.Structure):     # struct lh_llama_layer
        _fields_ = [(n, u64) for n in ("attention_norm", "wq", "wk", "wv", "wo", "ffn_norm", "w1", "w2", "w3")]

    class Desc(C.Structure):      # struct lh_llama_desc
        _fields_ = [(n, C.c_uint32) for n in ("vocab", "embd", "heads", "layers", "ff", "ctx", "layer0", "layer1")] + \
                   [("tok_embeddings", u64), ("norm", u64), ("output", u64), ("layer", C.POINTER(Layer)), ("k_cache", u64), ("v_cache", u64), ("weight_dtype", C.c_int)]

    lh.lh_last_error.restype = C.c_char_p
    lh.lh_last_error.argtypes = [VP]
    lh.lh_ctx_create.argtypes = [C.c_int, VP, C.POINTER(VP)]
    lh.lh_ctx_destroy.argtypes = [VP]
    lh.lh_tensor_register.argtypes = [VP, u64, C.c_int, u32p, C.c_int, VP, C.POINTER(u64)]
    lh.lh_buf_free.argtypes = [VP, u64]
    lh.lh_llama_create.argtypes = [VP, C.POINTER(Desc), C.POINTER(VP)]
    lh.lh_llama_destroy.argtypes = [VP]
    lh.lh_batch_create.argtypes = [VP, C.POINTER(VP), C.c_uint32, C.POINTER(VP)]
    lh.lh_batch_destroy.argtypes = [VP]
    lh.lh_batch_set.argtypes = [VP, u32p, u32p]
    lh.lh_batch_fork.argtypes = [VP, C.c_uint32, u32p, C.c_uint32, C.c_uint32]
    lh.lh_batch_share_info.argtypes = [VP, u32p, u32p]
    Vs, d, F, ctx_size = 64, 128, 256, 16
    ctx = VP()
    assert lh.lh_ctx_create(0, None, C.byref(ctx)) == 0, lh.lh_last_error(None)
    rng = np.random.default_rng(1)
    bufs = []

    def reg(shape, host=True):
        rows, cols = shape
        arr = (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32) if host else None
        ne = (C.c_uint32 * 4)(cols, rows, 1, 1)
        out = u64()
        assert lh.lh_tensor_register(ctx, 0, 0, ne, 1, arr.ctypes.data if host else None, C.byref(out)) == 0, lh.lh_last_error(ctx)
        bufs.append(out.value)
        return out.value

    layers = (Layer * 2)()
    layers[0] = Layer(reg((1, d)), reg((d, d)), reg((d, d)), reg((d, d)), reg((d, d)), reg((1, d)), reg((F, d)), reg((d, F)), reg((F, d)))
    emb = reg((Vs, d))
    pods = (VP * 2)()
    for i in range(2):
        desc = Desc(Vs, d, 1, 2, F, ctx_size, 0, 1, emb, 0, 0, layers, reg((1, d * ctx_size), host=False), reg((1, d * ctx_size), host=False), 0)
        pod = VP()
        assert lh.lh_llama_create(ctx, C.byref(desc), C.byref(pod)) == 0, lh.lh_last_error(ctx)
        pods[i] = pod.value
    b = VP()
    assert lh.lh_batch_create(ctx, pods, 2, C.byref(b)) == 0, lh.lh_last_error(ctx)
    try:
        toks, past = (C.c_uint32 * 2)(3, 5), (C.c_uint32 * 2)(4, 4)
        assert lh.lh_batch_set(b, toks, past) == 0, lh.lh_last_error(ctx)
        dst = (C.c_uint32 * 1)(1)
        assert lh.lh_batch_fork(b, 0, dst, 1, 2) == -4, "LH_EUNSUPPORTED"
        assert b"whole-model" in lh.lh_last_error(ctx)
        g, ln = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
        assert lh.lh_batch_share_info(b, g, ln) == 0 and list(g) == [0, 1] and list(ln) == [0, 0]
    finally:
        lh.lh_batch_destroy(b)
        for i in range(2):
            lh.lh_llama_destroy(pods[i])
        for bf in bufs:
            lh.lh_buf_free(ctx, bf)
        lh.lh_ctx_destroy(ctx)
