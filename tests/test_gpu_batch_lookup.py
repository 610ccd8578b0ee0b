"""-m gpu: lookup-draft speculative decoding for the pods of a batch (lh_batch_decode_lookup, lh_spec_accept_pods; kernels_spec.h).

Every check is an equality:
 1. the accept step alone (k_spec_accept_pods) == the rule of tests/batch_lookup_ref.py at 1, 3 and 64 pods;
 2. where the rows of a pass are bit-identical to solo rows (P * R <= 8 fp32, <= 4 block-int8) the loop == lh_batch_decode: ids, fp32 last logits byte for
    byte, per-pod stats and trace == the simulation, and the state left behind gives the same next tick;
 3. for any row count the loop == a host replay that feeds the same P * R rows through Batch.Feed with the per-row attention kernels, takes np.argmax per
    row and accepts by the Python rule: ids, traces, final positions, fp32 final logits rows byte for byte;
 4. a cycle model where one pod accepts whole drafts and the other none;
 5. the 7B matrix shapes, 8 rows against lh_batch_decode and 64 rows (k_stream_b9) against the replay;
 6. pod counts that leave no room for a second row: plain ticks, stats.rows == 1;
 7. every refusal leaves the batch as it was.
Every loop test asserts stats.rows: a silent fall-back to plain ticks fails."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_lookup_ref as bref          # noqa: E402
import speculative_ref as ref            # noqa: E402
import test_gpu_speculative as solo      # noqa: E402  (its small models: HD128, the cycle model, the 7B matrix shapes)
from llama_go_amd.mlapi import PROMPT, Batch, MLError, route_trace, spec_accept_pods   # noqa: E402

pytestmark = pytest.mark.gpu

HD128, NAN_TOKEN = solo.HD128, solo.NAN_TOKEN
V = HD128["vocab"]


@pytest.fixture(scope="module")
def pool(product):
    p = solo.Pool(product)
    yield p
    p.close()


def prompts_for(pods, vocab=V, seed=3):
    """different prompts of different lengths per pod"""
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, min(vocab, NAN_TOKEN), 6 + i % 3)] for i in range(pods)]


# ---- 1. the accept step against the Python rule -----------------------------------------------------------------------------------------------
def accept_cases(R, n_steps, ctx):
    """(arg, tok, k, pos, produced) of single pods"""
    rng = np.random.default_rng(R)
    cases = []

    def add(k, cut=None, later=False, pos=10, produced=0, filler_match=False):
        arg = [int(t) for t in rng.integers(100, 400, R)]
        pending = 7
        tok = [pending] + arg[:k] + [pending] * (R - 1 - k)          # the model's own continuation as the draft: accepted whole
        if cut is not None and cut < k:
            tok[cut + 1] = arg[cut + 1] if later and cut + 1 < R else 450 + cut   # wrong at `cut`: a later id of the run, or an id the run does not hold
        if filler_match and k + 1 < R:
            arg[k] = pending                                            # the first filler row "matches": it never counts
        cases.append((arg, tok[:R], k, pos, produced))
    K = R - 1
    add(0)
    add(K)
    if K >= 1:
        for cut in sorted({0, K // 2, K - 1}):
            add(K, cut)
            add(K, cut, later=True)
        add(K, pos=10, produced=n_steps - min(3, R))                   # clipped by remaining - 1
        add(K, pos=ctx - 2)                                            # clipped by the window
        add(max(K - 2, 0), filler_match=True)
    add(K, produced=n_steps)                                           # finished: changes nothing
    add(0, produced=n_steps)
    add(0, pos=10, produced=n_steps - 1)                               # its last id
    return cases


@pytest.mark.parametrize("pods,R", [(1, 8), (3, 8), (3, 4), (64, 1), (16, 4)])
def test_accept_pods_equals_the_python_rule(product, pods, R):
    n_steps, ctx = 40, 64
    cases = accept_cases(R, n_steps, ctx)
    cases = [cases[j % len(cases)] for j in range(-(-len(cases) // pods) * pods)]   # the cases again and again until they fill whole calls of `pods` pods
    fired = set()
    for c0 in range(0, len(cases), pods):
        grp = cases[c0:c0 + pods]
        assert len(grp) == pods
        a, pos, produced, pending, ids = spec_accept_pods(product, [c[0] for c in grp], [c[1] for c in grp], [c[2] for c in grp], [c[3] for c in grp],
                                                          [c[4] for c in grp], n_steps, ctx)
        for i, (arg, tok, k, p, pr) in enumerate(grp):
            want = bref.accept(arg, tok, k, p, pr, n_steps, ctx)
            assert (a[i], pos[i], produced[i], pending[i], ids[i]) == want, (pods, R, c0 + i, grp[i], want)
            fired.add("finished" if pr >= n_steps else "full" if want[0] == k else "cut")
    assert fired == ({"finished", "full", "cut"} if R > 1 else {"finished", "full"})
    if pods == 1:
        for bad in (dict(P=0, R=1), dict(P=65, R=1), dict(P=1, R=9), dict(P=9, R=8)):
            with pytest.raises(MLError):
                spec_accept_pods(product, np.zeros((bad["P"], bad["R"]), np.uint32), np.zeros((bad["P"], bad["R"]), np.uint32), [0] * bad["P"], [0] * bad["P"],
                                 [0] * bad["P"], n_steps, ctx)


# ---- the undisturbed run of a batch: lh_batch_decode -----------------------------------------------------------------------------------------
def batch_greedy(model, ctx, prompts, n):
    """(per pod g[0..n): g[0] = the id behind the prompt, the rest from lh_batch_decode; the last tick's logits; the ids of one more tick)"""
    b = Batch(model, ctx, len(prompts))
    g, lg = b.GreedyDecode(prompts, n, want_logits=True)
    more = b.Tick()
    b.free()
    return g, lg, more


def check_against_simulation(prompts, g, n, R, corpus, ctx, vocab, stats, traces, gmax=3, gmin=1):
    want = bref.simulate_pods([list(p) + [gi[0]] for p, gi in zip(prompts, g)], [gi[1:] for gi in g], n - 1, R, gmax, gmin, corpus, ctx, vocab)
    for i, (tr, st) in enumerate(want):
        assert traces[i] == tr and stats[i] == st, (i, traces[i], tr, stats[i], st)
    return want


# ---- 2. equals lh_batch_decode where the rows are bit-identical -------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", [256, 384])
@pytest.mark.parametrize("int8,pods,K", [(False, 2, 3), (False, 4, 1), (False, 1, 7), (True, 2, 1), (True, 1, 3)],
                         ids=["f32-2x4", "f32-4x2", "f32-1x8", "q8-2x2", "q8-1x4"])
def test_loop_equals_batch_decode_on_bit_identical_rows(pool, ctx, int8, pods, K):
    model, n, R = pool.model("hd128", ctx, int8), 33, K + 1
    prompts = prompts_for(pods)
    g, lg_last, more = batch_greedy(model, ctx, prompts, n)
    for i, p in enumerate(prompts):                                    # ... and each pod's solo greedy run
        assert g[i] == pool.greedy("hd128", ctx, int8, p, n)[0], i
    replay = [t for p, gi in zip(prompts, g) for t in list(p) + gi]
    bad = list(replay)
    for i in range(5, len(bad), 5):                                    # wrong at every fifth id: partial acceptance
        bad[i] = (bad[i] + 1) % NAN_TOKEN
    b = Batch(model, ctx, pods)
    for corpus, gmax in ((replay, 3), (None, 3), (bad, 2)):
        first = b.Prompt(prompts)
        assert first == [gi[0] for gi in g]
        ids, lg, stats, traces = b.DecodeLookup(first, [len(p) for p in prompts], n - 1, K, gmax, 1, corpus, want_logits=True)
        assert all(st["rows"] == R for st in stats), stats
        assert ids == [gi[1:] for gi in g]
        if not int8:
            assert lg.tobytes() == lg_last.tobytes(), "last logits"
        check_against_simulation(prompts, g, n, R, corpus, ctx, V, stats, traces, gmax)
        if corpus is replay:
            assert sum(st["accepted"] for st in stats) > 0
        if corpus is bad and K >= 3:
            assert any(a < k for tr in traces for k, a in tr), traces
        assert b.Tick() == more, "the state left behind"
    b.free()


# ---- 3. equals a host replay through Batch.Feed, for any row count ------------------------------------------------------------------------------
def feed_replay(b2, prompts, first, n_steps, R, gmax, gmin, corpus, ctx, vocab):
    """The loop on the host: per pass every pod drafts by the Python rule, the P * R rows [pending, draft, filler] go through ONE batched pass of
    Batch.Feed (per-row attention kernels), np.argmax per row, the Python accept rule.  A finished pod's rows stay as they were in its finishing pass.
    -> (ids, traces, positions, the logits behind each pod's last id, passes)"""
    P = len(prompts)
    H = [list(p) + [f] for p, f in zip(prompts, first)]
    pos, produced = [len(p) for p in prompts], [0] * P
    ids, traces, last = [[] for _ in range(P)], [[] for _ in range(P)], [None] * P
    toks, at, passes = [None] * P, list(pos), 0
    while min(produced) < n_steps:
        ks = [0] * P
        for i in range(P):
            if produced[i] >= n_steps:
                continue
            d = ref.draft(H[i], R - 1, gmax, gmin, corpus, min(ctx - len(H[i]), n_steps - produced[i] - 1), vocab)
            ks[i], toks[i], at[i] = len(d), [H[i][-1]] + d + [H[i][-1]] * (R - 1 - len(d)), pos[i]
        (_, rows), tr = route_trace(lambda: b2.Feed(toks, at, want_rows=True))
        assert [e for e in tr if e.startswith("feed_pass/")] == [f"feed_pass/batched/n{P * R}"], tr
        assert not [e for e in tr if "_seg" in e], tr                  # the per-row attention kernels
        arg = np.argmax(rows, axis=1).reshape(P, R)
        for i in range(P):
            if produced[i] >= n_steps:
                continue
            a, pos[i], produced[i], _, got = bref.accept(arg[i], toks[i], ks[i], pos[i], produced[i], n_steps, ctx)
            traces[i].append((ks[i], a))
            ids[i] += got
            H[i] += got
            if produced[i] >= n_steps:
                last[i] = rows[i * R + a].copy()
        passes += 1
    return ids, traces, pos, np.stack(last), passes


def run_against_replay(monkeypatch, model, ctx, int8, pods, K, R, n_steps, prompts, vocab, gmax=3):
    solo_runs = []
    for p in prompts[:4]:                                              # a corpus with something to find: a few pods' solo greedy runs
        c = model.NewContext(ctx, 1)
        solo_runs += list(p) + c.GreedyDecode(p, n_steps + 1, want_logits=False)[0]
        c.free()
    b = Batch(model, ctx, pods)
    first = b.Prompt(prompts)
    (ids, lg, stats, traces), tr = route_trace(lambda: b.DecodeLookup(first, [len(p) for p in prompts], n_steps, K, gmax, 1, solo_runs, want_logits=True))
    assert all(st["rows"] == R for st in stats), (R, stats)
    more = b.Tick()
    b.free()
    monkeypatch.setenv("LLAMAHIP_FEED_ROW_ATTN", "1")
    b2 = Batch(model, ctx, pods)
    assert b2.Prompt(prompts) == first
    want_ids, want_traces, want_pos, want_lg, passes = feed_replay(b2, prompts, first, n_steps, R, gmax, 1, solo_runs, ctx, vocab)
    assert ids == want_ids and traces == want_traces
    assert [st["passes"] for st in stats] == [len(t) for t in want_traces] and max(st["passes"] for st in stats) == passes
    assert sum(st["accepted"] for st in stats) > 0, stats
    if not int8:
        assert lg.tobytes() == want_lg.tobytes(), "the logits behind every pod's last id"
    # final positions: the next tick of both batches evaluates every pod's last id at past + n_steps
    b2.Set([t[-1] for t in want_ids], want_pos)
    assert want_pos == [len(p) + n_steps for p in prompts] and b2.Tick() == more
    b2.free()
    return tr


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
@pytest.mark.parametrize("ctx,pods,K,R", [(256, 3, 2, 3), (384, 5, 3, 4), (256, 8, 7, 8), (384, 9, 7, 7)], ids=["3x3", "5x4", "8x8", "9x7"])
def test_loop_equals_a_feed_replay_for_any_row_count(pool, monkeypatch, ctx, int8, pods, K, R):
    run_against_replay(monkeypatch, pool.model("hd128", ctx, int8), ctx, int8, pods, K, R, 24, prompts_for(pods), V)


# ---- 4. the cycle model -----------------------------------------------------------------------------------------------------------------------
def test_cycle_model_one_pod_accepts_everything_the_other_nothing(product):
    ctx, n, K = 64, 41, 4
    m, sigma = solo.cycle_model(product, ctx)
    prompts, g = [[3, 4, 10], [3, 4, 20]], []
    for p in prompts:
        run = [sigma[p[-1]]]
        while len(run) < n:
            run.append(sigma[run[-1]])
        g.append(run)
    b = Batch(m, ctx, 2)
    first = b.Prompt(prompts)
    assert first == [g[0][0], g[1][0]]
    ids, lg, stats, traces = b.DecodeLookup(first, [3, 3], n - 1, K, 3, 1, None, want_logits=True)
    b.free()
    m.free()
    assert ids == [g[0][1:], g[1][1:]] and all(st["rows"] == K + 1 for st in stats), stats
    check_against_simulation(prompts, g, n, K + 1, None, ctx, ref.UNKNOWN, stats, traces)
    # pod 0 inside the 5-cycle: four warm-up passes, then whole drafts; pod 1 on the long cycle: every draft empty, one id per pass
    assert traces[0][:4] == [(0, 0)] * 4 and all(t == (4, 4) for t in traces[0][4:-1]) and stats[0]["passes"] == 4 + 7 + 1
    assert stats[1]["empty"] == stats[1]["passes"] == n - 1 and stats[1]["drafted"] == 0
    # the logits behind each pod's last id are those of ITS finishing pass: one-hot at the id, whatever the 28 later passes of pod 1 did
    for i in range(2):
        assert int(np.argmax(lg[i])) == ids[i][-1] and np.count_nonzero(lg[i]) == 1, i


# ---- 5. the 7B matrix shapes ------------------------------------------------------------------------------------------------------------------
def prompts_7b(pods):
    return [[PROMPT[0]] + [(t + 17 * i) % 32000 for t in PROMPT[1:]] for i in range(pods)]


def test_7b_shapes_eight_rows_equal_batch_decode(pool):
    ctx, n, pods, K = 64, 24, 4, 1
    model = pool.model("7b", ctx, False)
    prompts = prompts_7b(pods)
    g, lg_last, more = batch_greedy(model, ctx, prompts, n)
    replay = [t for p, gi in zip(prompts, g) for t in list(p) + gi]
    b = Batch(model, ctx, pods)
    first = b.Prompt(prompts)
    ids, lg, stats, traces = b.DecodeLookup(first, [len(p) for p in prompts], n - 1, K, 3, 1, replay, want_logits=True)
    assert all(st["rows"] == K + 1 for st in stats) and ids == [gi[1:] for gi in g] and lg.tobytes() == lg_last.tobytes()
    check_against_simulation(prompts, g, n, K + 1, replay, ctx, 32000, stats, traces)
    assert b.Tick() == more
    b.free()


def test_7b_shapes_sixty_four_rows_equal_the_feed_replay(pool, monkeypatch):
    ctx, pods, K = 64, 8, 7
    tr = run_against_replay(monkeypatch, pool.model("7b", ctx, False), ctx, False, pods, K, 8, 16, prompts_7b(pods), 32000)
    assert any(e.startswith("k_stream_b9") for e in tr), tr          # the first (eager) pass names its route


# ---- 6. no room for a second row --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pods", [33, 64])
def test_too_many_pods_for_a_second_row_take_plain_ticks(pool, pods):
    ctx, n = 256, 9
    model = pool.model("hd128", ctx, False)
    prompts = prompts_for(pods)
    g, lg_last, more = batch_greedy(model, ctx, prompts, n)
    b = Batch(model, ctx, pods)
    first = b.Prompt(prompts)
    ids, lg, stats, traces = b.DecodeLookup(first, [len(p) for p in prompts], n - 1, 7, 3, 1, None, want_logits=True)
    assert all(st == dict(passes=n - 1, rows=1, drafted=0, accepted=0, empty=n - 1) for st in stats), stats[0]
    assert all(tr == [(0, 0)] * (n - 1) for tr in traces)
    assert ids == [gi[1:] for gi in g] and lg.tobytes() == lg_last.tobytes() and b.Tick() == more
    b.free()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_refusals_leave_the_batch_as_it_was(pool, int8):
    ctx, pods, K = 64, 2, 1
    R = K + 1
    model = pool.model("hd128", ctx, int8)
    prompts = prompts_for(pods)
    past = [len(p) for p in prompts]
    n_edge = ctx - max(past) - R + 1                                   # max(past) + n_edge + R - 1 == ctx
    g, _, _ = batch_greedy(model, ctx, prompts, n_edge + 1)
    b = Batch(model, ctx, pods)
    first = b.Prompt(prompts)
    with pytest.raises(MLError, match="exceeds the context window"):
        b.DecodeLookup(first, past, n_edge + 1, K)                     # one position past the boundary
    with pytest.raises(MLError, match="exceeds the context window"):
        b.DecodeLookup(first, [past[0], ctx], 1, K)
    for kw in (dict(draft_max=0), dict(draft_max=8), dict(draft_max=K, ngram_min=0), dict(draft_max=K, ngram_max=2, ngram_min=3), dict(draft_max=K, ngram_max=9),
               dict(draft_max=K, corpus=[1] * 65537), dict(draft_max=K, corpus=[1, 2, V, 3])):
        with pytest.raises(MLError):
            b.DecodeLookup(first, past, 4, **kw)
    with pytest.raises(MLError):
        b.DecodeLookup(first, past, 0, K)
    with pytest.raises(MLError):
        b.DecodeLookup([first[0], V], past, 4, K)                      # a first token outside the vocabulary
    # the batch stands behind its prompts as if nothing had been asked of it: its ticks give the undisturbed ids of lh_batch_decode
    assert [b.Tick() for _ in range(4)] == [[gi[1 + t] for gi in g] for t in range(4)]
    b.SetSampler(seed=1)
    with pytest.raises(MLError, match="sampler"):
        b.DecodeLookup(first, past, 4, K)
    b.ClearSampler()
    assert [b.Tick() for _ in range(4)] == [[gi[5 + t] for gi in g] for t in range(4)]
    # ... and the loop AT the boundary, from the prompts again, gives the same run
    ids, _, stats, _ = b.DecodeLookup(first, past, n_edge, K, corpus=[t for gi in g for t in gi])
    assert all(st["rows"] == R for st in stats) and ids == [gi[1:] for gi in g]
    b.free()
