"""-m gpu: lookup-draft speculative decoding for the pods of a SAMPLING batch (lh_batch_decode_sample_lookup, lh_sample_pod_rows,
lh_spec_accept_sample_pods, lh_batch_sampler_read; k_sample_pod_rows / k_sample_small_pod_rows, the sampled commit of k_spec_accept_pods).

The device sampler's uniforms are counter-based, so every check is an equality:
 1. one sampler launch over pods x rows == the checker per row over the Python ring view as call draw_i + r; rows behind a draft stay 0xFFFFFFFF; pods
    see their own rings; the refusals;
 2. the accept step with the ring commit == the rule of tests/batch_sample_lookup_ref.py at 1, 3 and 64 pods, rings slot for slot;
 3. where the rows of a pass are bit-identical to solo rows the loop == sampled lh_batch_decode: ids, fp32 last logits byte for byte, stats and traces ==
    the simulation, every pod's sampler state, the next sampled tick;  4. ... and each pod's ids == its solo SampleDecode run;
 5. for any row count the loop == a host replay through Batch.Feed of a greedy twin batch (per-row attention kernels), the checker sampling every row;
 6. the 7B matrix shapes: 8 rows against lh_batch_decode, 64 rows (k_stream_b9) against the replay;
 7. the cycle model with topK 1: one pod accepts whole drafts, the other none, rings and draws still those of the ticks;
 8. pod counts without room for a second row take plain sampled ticks;
 9. every refusal leaves batch and sampler state as they were; a batch of layer-shard stages, built through the C-ABI as the cgo shim builds its stages
    (the host mirror only builds whole-model batches), is refused with LH_EUNSUPPORTED on a first and on a last stage;
10. LLAMAHIP_NO_GRAPH=1 == the captured run.
Every loop test asserts stats.rows: a silent fall-back to plain ticks fails."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_sample_lookup_ref as bsref    # noqa: E402
import feed_sample_ref as fr               # noqa: E402
import sample_lookup_cases as sc           # noqa: E402
import speculative_ref as ref              # noqa: E402
import test_gpu_batch_lookup as greedy     # noqa: E402  (accept_cases, check_against_simulation, prompts_7b)
import test_gpu_speculative as solo        # noqa: E402  (its small models: HD128, the cycle model, the 7B matrix shapes)
from test_gpu_feed_sample import SEED, SMP, checker_sampler   # noqa: E402
from llama_go_amd.mlapi import FEED_NEW, Batch, MLError, lookup_params, route_trace, sample_pod_rows, spec_accept_sample_pods   # noqa: E402

pytestmark = pytest.mark.gpu

HD128, NAN_TOKEN = solo.HD128, solo.NAN_TOKEN
V = HD128["vocab"]
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def octx(oracle):
    return oracle.NewContext(1)


@pytest.fixture(scope="module")
def pool(product):
    p = solo.Pool(product)
    yield p
    p.close()


# ---- 1. the sampler launch over pods x rows ---------------------------------------------------------------------------------------------------
PR = [(1, 8), (3, 4), (8, 8), (64, 1), (16, 4)]


def pod_rows_case(rng, Vn, P, R, rs):
    """P * R rows; per pod a ring of rs slots at its own fill, a draft of its own length made mostly of ids from its rows' top places (where the penalty
    changes the answer), its own draw."""
    lg = np.stack([sc.logits_of(rng, Vn, ("normal", "ties", "normal", "neginf")[e % 4]) for e in range(P * R)])
    rings, pos, toks, nd = [], [], [], []
    for i in range(P):
        hot = np.argsort(-lg[i * R], kind="stable")[:4]
        pick = lambda: int(hot[rng.integers(0, len(hot))]) if rng.random() < 0.7 else int(rng.integers(0, Vn))   # noqa: E731
        cnt = (0, rs // 2, rs, 3 * rs + 2, 1)[(i + rs) % 5]
        ring, p = sc.ring_after([pick() for _ in range(cnt)], rs)
        rings.append(ring)
        pos.append(p)
        k = (R - 1, 0, (R - 1) // 2, R - 1, max(R - 2, 0))[i % 5]
        pending = pick()
        toks.append([pending] + [pick() for _ in range(k)] + [pending] * (R - 1 - k))
        nd.append(k)
    return lg, rings, pos, [int(d) for d in rng.integers(0, 1 << 40, P)], toks, nd


def check_pod_rows(product, sample, lg, rings, pos, draws, toks, nd, **kw):
    got = sample_pod_rows(product, lg, rings, pos, draws, toks, nd, seed=SEED, **dict(SMP, **kw))
    R = len(toks[0])
    for i in range(len(toks)):
        for r in range(R):
            want = int(sample(lg[i * R + r], sc.ring_view(rings[i], pos[i], toks[i], r), draws[i] + r)) if r <= nd[i] else NONE
            assert int(got[i][r]) == want, (i, r, int(got[i][r]), want, rings[i], pos[i], toks[i], nd[i])
    return got


@pytest.mark.parametrize("Vn", [63, 1000, 1025, 32000])
def test_pod_rows_launch_equals_the_checker_per_row(product, oracle, octx, Vn):
    """Both kernels (topK 1 | 40 -> k_sample_small_pod_rows, 65 -> k_sample_pod_rows), the 4-byte load path (V % 4 != 0), every (pods, rows) shape, ring
    sizes 1, 5 and 64 (ring_size < row included) at several fills."""
    rng = np.random.default_rng(Vn)
    case = 0
    for topK in (1, 40, min(65, Vn)):
        sample = checker_sampler(oracle, octx, topK=topK)
        for P, R in PR:
            if Vn == 32000 and P * R == 64 and (topK == 1 or (topK != 40 and R == 1)):
                continue                                            # (64 x 32000 on the checker: both shapes on the small kernel, 8 x 8 on the general one)
            rs = (1, 5, 64)[case % 3]
            case += 1
            check_pod_rows(product, sample, *pod_rows_case(rng, Vn, P, R, rs), topK=topK)


@pytest.mark.parametrize("topK,topP", [(1, 0.95), (65, 0.01)])     # the deterministic settings of both kernels
def test_pod_rows_see_their_own_rings_and_drafts(product, oracle, octx, topK, topP):
    """t is the maximum by a small margin, u the runner-up; a row answers u exactly when t is in ITS pod's ring or in the draft in front of IT."""
    Vn, t, u = 1000, 700, 5
    row = np.full(Vn, -30.0, np.float32)
    row[t], row[u] = 10.0, 9.9
    lg = np.stack([row] * 9)
    rings = [[30, 31, 32, 33], [30, 31, 32, 33], [30, t, 32, 33]]
    toks = [[40, 41, 42], [40, t, 42], [40, 41, 42]]
    kw = dict(topK=topK, topP=topP, temp=1.0, repeatPenalty=1.5)
    got = check_pod_rows(product, checker_sampler(oracle, octx, **kw), lg, rings, [4, 4, 6], [3, 0, 9], toks, [2, 2, 2], **kw)
    assert got.tolist() == [[t, t, t], [t, u, u], [u, u, u]]
    # one slot: the draft in front of a row overwrites it
    got = check_pod_rows(product, checker_sampler(oracle, octx, **kw), lg[:6], [[t], [t]], [1, 1], [0, 5], [[40, 41, 42], [t, t, 42]], [2, 1], **kw)
    assert got.tolist() == [[u, t, t], [u, u, NONE]]


def test_sample_pod_rows_refusals(product):
    Vn = 1000
    ok = dict(SMP)

    def call(P, R, Vv=Vn, rs=2, tok=None, **kw):
        return sample_pod_rows(product, np.zeros((P * R, Vv), np.float32), np.ones((P, rs), np.uint32), [0] * P, [0] * P,
                               np.zeros((P, R), np.uint32) if tok is None else tok, [0] * P, **dict(ok, **kw))
    assert call(2, 3).shape == (2, 3)
    for P, R in ((0, 1), (65, 1), (1, 9), (1, 0), (9, 8)):
        with pytest.raises(MLError, match="pods x"):
            call(P, R)
    with pytest.raises(MLError, match="vocabulary"):
        call(1, 1, Vv=65537)
    with pytest.raises(MLError, match="slot"):
        call(2, 2, rs=0)
    with pytest.raises(MLError, match="draft id"):
        call(2, 2, tok=np.array([[0, 1], [0, Vn]], np.uint32))
    for bad, msg in ((dict(topK=0), "topK"), (dict(topK=Vn + 1), "topK"), (dict(temp=0.0), "temp"), (dict(repeatPenalty=0.0), "repeatPenalty")):
        with pytest.raises(MLError, match=msg):
            call(2, 2, **bad)
    with pytest.raises(MLError, match="device limit"):
        call(1, 1, Vv=4000, topK=2000)
    f = product.lib.llamago_SamplePodRows
    u32p, f32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    lg = np.zeros((2, Vn), np.float32)
    two, dr, out = (C.c_uint32 * 2)(0, 1), (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 64)()
    args = [lg.ctypes.data_as(f32p), 2, 1, Vn, C.cast(two, u32p), 1, C.cast(two, u32p), C.cast(dr, u64p), C.cast(two, u32p), C.cast(two, u32p), 40, 0.95, 0.8, 1.1, 1,
            C.cast(out, u32p)]
    assert f(*args) == 0
    for i in (0, 4, 6, 7, 8, 9, 15):
        a = list(args)
        a[i] = None
        assert f(*a) != 0 and b"null" in product.lib.ml_LastError(), i


# ---- 2. the accept step with the commit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pods,R", [(1, 8), (3, 8), (3, 4), (64, 1), (16, 4)])
def test_accept_sample_pods_equals_the_python_rule(product, pods, R):
    n_steps, ctx = 40, 64
    cases = greedy.accept_cases(R, n_steps, ctx)
    cases = [cases[j % len(cases)] for j in range(-(-len(cases) // pods) * pods)]
    rng = np.random.default_rng(pods * 10 + R)
    fired = set()
    for c0 in range(0, len(cases), pods):
        grp = cases[c0:c0 + pods]
        for rs in (1, 5, 64):                                          # ring_size < a + 1 included
            rings = rng.integers(1, 500, (pods, rs)).astype(np.uint32)
            rpos = [int(x) for x in rng.integers(0, 3 * rs + 1, pods)]
            draws = [int(x) for x in rng.integers(0, 1 << 40, pods)]
            a, pos, produced, pending, ids, rout, rpo, dro = spec_accept_sample_pods(product, [c[0] for c in grp], [c[1] for c in grp], [c[2] for c in grp],
                                                                                     [c[3] for c in grp], [c[4] for c in grp], n_steps, ctx, rings, rpos, draws)
            for i, (arg, tok, k, p, pr) in enumerate(grp):
                pod = fr.Pod(rs, rings[i], rpos[i], draws[i])
                want = bsref.accept_commit(pod, arg, tok, k, p, pr, n_steps, ctx)
                assert (a[i], pos[i], produced[i], pending[i], ids[i]) == want, (pods, R, rs, c0 + i, grp[i], want)
                assert ([int(t) for t in rout[i]], rpo[i], dro[i]) == (pod.ring, pod.ring_pos, pod.draw), (pods, R, rs, c0 + i, "ring, ring_pos, draw")
                if pr >= n_steps:
                    assert pod.key() == (tuple(int(t) for t in rings[i]), rpos[i], draws[i])
                fired.add("finished" if pr >= n_steps else "full" if want[0] == k else "cut")
                if rs < want[0] + 1:
                    fired.add("wrapped")
    assert fired >= ({"finished", "full", "cut", "wrapped"} if R > 1 else {"finished", "full"})
    if pods == 1:
        z = np.zeros((1, 1), np.uint32)
        with pytest.raises(MLError, match="slot"):
            spec_accept_sample_pods(product, z, z, [0], [0], [0], n_steps, ctx, np.zeros((1, 0), np.uint32), [0], [0])
        for P, Rr in ((0, 1), (65, 1), (1, 9), (9, 8)):
            with pytest.raises(MLError):
                spec_accept_sample_pods(product, np.zeros((P, Rr), np.uint32), np.zeros((P, Rr), np.uint32), [0] * P, [0] * P, [0] * P, n_steps, ctx,
                                        np.ones((max(P, 1), 2), np.uint32)[:P], [0] * P, [0] * P)


# ---- the undisturbed run of a sampling batch: SetSampler, FeedSample(NEW + prompt), lh_batch_decode -------------------------------------------------
def short_prompts(pods, rows, vocab=V, seed=3):
    """different prompts of `rows` tokens in all (8 fp32 / 4 block-int8: the fed pass is bit-identical to solo prompt Evals)"""
    rng = np.random.default_rng(seed)
    lens = [rows // pods + (1 if i < rows % pods else 0) for i in range(pods)]
    return [[int(t) for t in rng.integers(0, min(vocab, NAN_TOKEN), n)] for n in lens]


def start(b, prompts, ctx, smp):
    """a new job on every pod: the rings hold the prompts and the first ids -> the first ids (pending)"""
    b.SetSampler(ringSize=ctx, **smp)
    return b.FeedSample(prompts, [0] * len(prompts), [FEED_NEW] * len(prompts))


def tick_run(model, ctx, prompts, n, smp):
    """-> (per pod g[0..n): g[0] the id behind the prompt, the rest from sampled lh_batch_decode; the last tick's logits; every pod's sampler state; the
    ids of one more tick)"""
    b = Batch(model, ctx, len(prompts))
    first = start(b, prompts, ctx, smp)
    ids, lg = b.Decode(first, [len(p) for p in prompts], n - 1, want_logits=True)
    states = [b.SamplerState(i) for i in range(len(prompts))]
    more = b.Tick()
    b.free()
    return [[f] + i for f, i in zip(first, ids)], lg, states, more


def corrupted(replay):
    bad = list(replay)
    for i in range(5, len(bad), 5):                                    # wrong at every fifth id: partial acceptance
        bad[i] = (bad[i] + 1) % NAN_TOKEN
    return bad


def loop_equals_ticks(model, ctx, int8, prompts, n, K, smp, vocab, corpora=("replay", "none", "bad"), solo_run=None):
    R, pods, past = K + 1, len(prompts), [len(p) for p in prompts]
    g, lg_last, states, more = tick_run(model, ctx, prompts, n, smp)
    assert len({tuple(gi) for gi in g}) == pods or pods == 1, "the pods draw different ids"
    if solo_run is not None:
        for i, p in enumerate(prompts):                                # ... and each pod's solo sampled loop
            assert g[i] == solo_run(p), i
    replay = [t for p, gi in zip(prompts, g) for t in list(p) + gi]
    b = Batch(model, ctx, pods)
    for name in corpora:
        corpus, gmax = dict(replay=(replay, 3), none=(None, 3), bad=(corrupted(replay), 2))[name]
        first = start(b, prompts, ctx, smp)
        assert first == [gi[0] for gi in g]
        ids, lg, stats, traces = b.DecodeSampleLookup(first, past, n - 1, K, gmax, 1, corpus, want_logits=True)
        assert all(st["rows"] == R for st in stats), stats
        assert ids == [gi[1:] for gi in g], name
        if not int8:
            assert lg.tobytes() == lg_last.tobytes(), "the rows the last ids were sampled from"
        greedy.check_against_simulation(prompts, g, n, R, corpus, ctx, vocab, stats, traces, gmax)
        if name == "replay":
            assert sum(st["accepted"] for st in stats) > 0
        if name == "bad" and K >= 3:
            assert any(a < k for tr in traces for k, a in tr), traces
        assert [b.SamplerState(i) for i in range(pods)] == states, "rings, ring_pos and draws"
        assert b.Tick() == more, "the state left behind"
    b.free()
    return g


# ---- 3. + 4. equals sampled lh_batch_decode (and the solo loops) where the rows are bit-identical ---------------------------------------------------
@pytest.mark.parametrize("topK", [40, 100])
@pytest.mark.parametrize("ctx", [256, 384])
@pytest.mark.parametrize("int8,pods,K", [(False, 2, 3), (False, 4, 1), (False, 1, 7), (True, 2, 1), (True, 1, 3)],
                         ids=["f32-2x4", "f32-4x2", "f32-1x8", "q8-2x2", "q8-1x4"])
def test_loop_equals_sampled_batch_decode_on_bit_identical_rows(pool, ctx, int8, pods, K, topK):
    model, n = pool.model("hd128", ctx, int8), 33
    smp = dict(SMP, seed=SEED, topK=topK)

    def solo_run(prompt):
        c = model.NewContext(ctx, 1)
        run = c.SampleDecode(prompt, n, **smp)
        c.free()
        return run
    loop_equals_ticks(model, ctx, int8, short_prompts(pods, 4 if int8 else 8), n, K, smp, V, solo_run=solo_run)


# ---- 5. equals a host replay through Batch.Feed, for any row count ------------------------------------------------------------------------------
def feed_replay(b2, sample, prompts, first, n_steps, R, gmax, gmin, corpus, ctx, vocab):
    """The loop on the host: per pass every pod drafts by the Python rule, the P * R rows [pending, draft, filler] go through ONE batched pass of Batch.Feed
    of the greedy twin (per-row attention kernels), the checker samples every row r <= k_i over the Python ring view as call draw_i + r, accept and commit
    follow the Python rule.  A finished pod's rows stay as they were in its finishing pass.
    -> (ids, traces, positions, sampler states, the logits behind each pod's last id)"""
    P = len(prompts)
    H = [list(p) + [f] for p, f in zip(prompts, first)]
    pods = []
    for p, f in zip(prompts, first):                                   # NEW + prompt, then the first sampling call
        pod = fr.Pod(ctx)
        fr.feed_ring(pod, p, fr.FEED_NEW)
        bsref.commit(pod, [f])
        pods.append(pod)
    pos, produced = [len(p) for p in prompts], [0] * P
    ids, traces, last = [[] for _ in range(P)], [[] for _ in range(P)], [None] * P
    toks, at = [None] * P, list(pos)
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
        for i in range(P):
            if produced[i] >= n_steps:
                continue
            arg = bsref.sample_rows(pods[i], sample, rows[i * R:(i + 1) * R], toks[i], ks[i])
            a, pos[i], produced[i], _, got = bsref.accept_commit(pods[i], arg, toks[i], ks[i], pos[i], produced[i], n_steps, ctx)
            traces[i].append((ks[i], a))
            ids[i] += got
            H[i] += got
            if produced[i] >= n_steps:
                last[i] = rows[i * R + a].copy()
    return ids, traces, pos, [(p.ring, p.ring_pos, p.draw) for p in pods], np.stack(last)


def run_against_replay(monkeypatch, oracle, octx, model, ctx, int8, pods, K, R, n_steps, prompts, vocab, gmax=3):
    monkeypatch.setenv("LLAMAHIP_FEED_ROW_ATTN", "1")                  # both batches' prompts through the same launches: byte-equal caches
    smp = dict(SMP, seed=SEED)
    past = [len(p) for p in prompts]
    g, _, _, _ = tick_run(model, ctx, prompts, n_steps + 1, smp)       # a corpus with something to find: the tick run of the same batch
    corpus = [t for p, gi in zip(prompts, g) for t in list(p) + gi]
    b = Batch(model, ctx, pods)
    first = start(b, prompts, ctx, smp)
    (ids, lg, stats, traces), tr = route_trace(lambda: b.DecodeSampleLookup(first, past, n_steps, K, gmax, 1, corpus, want_logits=True))
    assert all(st["rows"] == R for st in stats), (R, stats)
    assert [e for e in tr if e.startswith("k_sample")][:1] == [f"k_sample_small_pod_rows/n{pods * R}"], tr
    states = [b.SamplerState(i) for i in range(pods)]
    more = b.Tick()
    b.free()
    sample = checker_sampler(oracle, octx)
    b2 = Batch(model, ctx, pods)
    b2.Feed(prompts, [0] * pods)
    want_ids, want_traces, want_pos, want_states, want_lg = feed_replay(b2, sample, prompts, first, n_steps, R, gmax, 1, corpus, ctx, vocab)
    # the device batch's positions and pending ids: its next sampled tick draws what the checker draws from the twin's rows of every pod's last id at the
    # replay's positions (one row per pod in one pass, the rows of a tick), over the replay's rings as the replay's next sampling calls
    _, rows = b2.Feed([[t[-1]] for t in want_ids], want_pos, want_rows=True)
    b2.free()
    assert more == [int(sample(rows[i], list(st[0]), st[2])) for i, st in enumerate(want_states)], "the next tick: positions and pending ids"
    assert ids == want_ids and traces == want_traces
    assert [st["passes"] for st in stats] == [len(t) for t in want_traces]
    assert sum(st["accepted"] for st in stats) > 0, stats
    assert want_pos == [p + n_steps for p in past] and states == want_states, "the replay's positions; rings, ring_pos and draws"
    if not int8:
        assert lg.tobytes() == want_lg.tobytes(), "the rows every pod's last id was sampled from"
    return tr


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
@pytest.mark.parametrize("ctx,pods,K,R", [(256, 3, 2, 3), (384, 5, 3, 4), (256, 8, 7, 8), (384, 9, 7, 7)], ids=["3x3", "5x4", "8x8", "9x7"])
def test_loop_equals_a_feed_replay_for_any_row_count(pool, oracle, octx, monkeypatch, ctx, int8, pods, K, R):
    run_against_replay(monkeypatch, oracle, octx, pool.model("hd128", ctx, int8), ctx, int8, pods, K, R, 24, greedy.prompts_for(pods), V)


# ---- 6. the 7B matrix shapes ------------------------------------------------------------------------------------------------------------------
def test_7b_shapes_eight_rows_equal_sampled_batch_decode(pool):
    ctx = 64
    prompts = [p[:4] for p in greedy.prompts_7b(2)]                    # 8 prompt rows: the fed pass is bit-identical too
    loop_equals_ticks(pool.model("7b", ctx, False), ctx, False, prompts, 24, 3, dict(SMP, seed=SEED), 32000, corpora=("replay",))


def test_7b_shapes_sixty_four_rows_equal_the_feed_replay(pool, oracle, octx, monkeypatch):
    ctx, pods, K = 64, 8, 7
    tr = run_against_replay(monkeypatch, oracle, octx, pool.model("7b", ctx, False), ctx, False, pods, K, 8, 16, greedy.prompts_7b(pods), 32000)
    assert any(e.startswith("k_stream_b9") for e in tr), tr          # the first (eager) pass names its route


# ---- 7. the cycle model -----------------------------------------------------------------------------------------------------------------------
def test_cycle_model_with_top_k_one_is_greedy(product):
    """topK 1: the sampler takes the penalised maximum, and a one-hot row keeps its maximum under the penalty (1 / 1.3 > 0): the ids are sigma's."""
    ctx, n, K = 64, 41, 4
    m, sigma = solo.cycle_model(product, ctx)
    prompts, g = [[3, 4, 10], [3, 4, 20]], []
    for p in prompts:
        run = [sigma[p[-1]]]
        while len(run) < n:
            run.append(sigma[run[-1]])
        g.append(run)
    smp = dict(SMP, seed=SEED, topK=1)
    gt, _, states, more = tick_run(m, ctx, prompts, n, smp)
    assert gt == g
    b = Batch(m, ctx, 2)
    first = start(b, prompts, ctx, smp)
    ids, lg, stats, traces = b.DecodeSampleLookup(first, [3, 3], n - 1, K, 3, 1, None, want_logits=True)
    assert ids == [g[0][1:], g[1][1:]] and all(st["rows"] == K + 1 for st in stats), stats
    greedy.check_against_simulation(prompts, g, n, K + 1, None, ctx, ref.UNKNOWN, stats, traces)
    assert traces[0][:4] == [(0, 0)] * 4 and all(t == (4, 4) for t in traces[0][4:-1]) and stats[0]["passes"] == 4 + 7 + 1
    assert stats[1]["empty"] == stats[1]["passes"] == n - 1 and stats[1]["drafted"] == 0
    assert [b.SamplerState(i) for i in range(2)] == states and b.Tick() == more
    for i in range(2):
        assert states[i][1] == 3 + n and states[i][2] == n
        assert int(np.argmax(lg[i])) == ids[i][-1] and np.count_nonzero(lg[i]) == 1, i
    b.free()
    m.free()


# ---- 8. no room for a second row --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pods", [33, 64])
def test_too_many_pods_for_a_second_row_take_plain_sampled_ticks(pool, pods):
    ctx, n = 256, 9
    model = pool.model("hd128", ctx, False)
    prompts = short_prompts(pods, 2 * pods)
    smp = dict(SMP, seed=SEED)
    g, lg_last, states, more = tick_run(model, ctx, prompts, n, smp)
    b = Batch(model, ctx, pods)
    first = start(b, prompts, ctx, smp)
    ids, lg, stats, traces = b.DecodeSampleLookup(first, [len(p) for p in prompts], n - 1, 7, 3, 1, None, want_logits=True)
    assert all(st == dict(passes=n - 1, rows=1, drafted=0, accepted=0, empty=n - 1) for st in stats), stats[0]
    assert all(tr == [(0, 0)] * (n - 1) for tr in traces)
    assert ids == [gi[1:] for gi in g] and lg.tobytes() == lg_last.tobytes()
    assert [b.SamplerState(i) for i in range(pods)] == states and b.Tick() == more
    b.free()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_refusals_leave_batch_and_sampler_as_they_were(pool, int8):
    ctx, pods, K = 64, 2, 1
    R = K + 1
    model = pool.model("hd128", ctx, int8)
    prompts = short_prompts(pods, 4)
    past = [len(p) for p in prompts]
    n_edge = ctx - max(past) - R + 1                                   # max(past) + n_edge + R - 1 == ctx
    smp = dict(SMP, seed=SEED)
    g, _, _, _ = tick_run(model, ctx, prompts, n_edge + 1, smp)
    b = Batch(model, ctx, pods)
    with pytest.raises(MLError, match="no sampler"):
        b.DecodeSampleLookup([1, 2], past, 4, K)                       # a greedy batch
    with pytest.raises(MLError, match="no sampler"):
        b.SamplerState(0)
    first = start(b, prompts, ctx, smp)
    before = [b.SamplerState(i) for i in range(pods)]
    assert all(st[1] == len(p) + 1 and st[2] == 1 and st[0][:len(p) + 1] == list(p) + [f] for st, p, f in zip(before, prompts, first)), "the rings hold the prompts"

    def refused(match, *a, **kw):
        with pytest.raises(MLError, match=match):
            b.DecodeSampleLookup(*a, **kw)
        assert [b.SamplerState(i) for i in range(pods)] == before
    refused("exceeds the context window", first, past, n_edge + 1, K)  # one position past the boundary
    refused("exceeds the context window", first, [past[0], ctx], 1, K)
    for kw in (dict(draft_max=0), dict(draft_max=8), dict(draft_max=K, ngram_min=0), dict(draft_max=K, ngram_max=2, ngram_min=3), dict(draft_max=K, ngram_max=9),
               dict(draft_max=K, corpus=[1] * 65537), dict(draft_max=K, corpus=[1, 2, V, 3])):
        refused(None, first, past, 4, **kw)
    refused("no ids", first, past, 0, K)
    refused("vocabulary", [first[0], V], past, 4, K)                   # a first token outside the vocabulary
    f = b.ml.lib.llamago_BatchDecodeSampleLookup
    for null_at in (1, 2, 4, 5):                                       # first_tokens, past, lookup parameters, out
        args = [b.h, (C.c_uint32 * 2)(*first), (C.c_uint32 * 2)(*past), 4, None, (C.c_uint32 * 8)(), None, None, None, 0]
        if null_at != 4:
            lp, _keep = lookup_params(K, 3, 1, None)
            args[4] = C.byref(lp)
            args[null_at] = None
        assert f(*args) != 0
        assert [b.SamplerState(i) for i in range(pods)] == before
    with pytest.raises(MLError, match="outside the batch"):
        b.SamplerState(pods)
    # the batch stands behind its prompts as if nothing had been asked of it: its sampled ticks give the undisturbed ids
    assert [b.Tick() for _ in range(4)] == [[gi[1 + t] for gi in g] for t in range(4)]
    # ... and the loop AT the boundary, from the prompts again, gives the same run
    first = start(b, prompts, ctx, smp)
    ids, _, stats, _ = b.DecodeSampleLookup(first, past, n_edge, K, corpus=[t for gi in g for t in gi])
    assert all(st["rows"] == R for st in stats) and ids == [gi[1:] for gi in g]
    b.free()


def test_refuses_a_batch_of_layer_shard_stages(product):
    """Layers [0, 1) (a first stage: no sampler can be armed there) and [1, 2) (a last stage: it samples) of a two-layer model, two pods each, built through
    the C-ABI.  lh_batch_decode_sample_lookup answers LH_EUNSUPPORTED before anything is enqueued: the last stage's rings, ring_pos and draws are what
    lh_batch_set_sampler left, and the tick behind the refused call gives what it gives without it - residual rows byte for byte on the first stage; ids
    and sampler state on the last one."""
    import torch
    import llama_go_amd as pkg
    from llama_go_amd.mlapi import LookupParams
    lh = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    VP, u32p, u64 = C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64

    class Layer(C.Structure):     # struct lh_llama_layer
        _fields_ = [(n, u64) for n in ("attention_norm", "wq", "wk", "wv", "wo", "ffn_norm", "w1", "w2", "w3")]

    class Desc(C.Structure):      # struct lh_llama_desc
        _fields_ = [(n, C.c_uint32) for n in ("vocab", "embd", "heads", "layers", "ff", "ctx", "layer0", "layer1")] + \
                   [("tok_embeddings", u64), ("norm", u64), ("output", u64), ("layer", C.POINTER(Layer)), ("k_cache", u64), ("v_cache", u64), ("weight_dtype", C.c_int)]

    class SampleParams(C.Structure):   # struct lh_sample_params
        _fields_ = [("top_k", C.c_uint32), ("top_p", C.c_float), ("temp", C.c_float), ("repeat_penalty", C.c_float), ("seed", u64)]

    lh.lh_last_error.restype = C.c_char_p
    lh.lh_last_error.argtypes = [VP]
    lh.lh_ctx_create.argtypes = [C.c_int, VP, C.POINTER(VP)]
    lh.lh_ctx_destroy.argtypes = [VP]
    lh.lh_ctx_sync.argtypes = [VP]
    lh.lh_tensor_register.argtypes = [VP, u64, C.c_int, u32p, C.c_int, VP, C.POINTER(u64)]
    lh.lh_buf_free.argtypes = [VP, u64]
    lh.lh_llama_create.argtypes = [VP, C.POINTER(Desc), C.POINTER(VP)]
    lh.lh_llama_destroy.argtypes = [VP]
    lh.lh_batch_create.argtypes = [VP, C.POINTER(VP), C.c_uint32, C.POINTER(VP)]
    lh.lh_batch_destroy.argtypes = [VP]
    lh.lh_batch_set.argtypes = [VP, u32p, u32p]
    lh.lh_batch_stage.argtypes = [VP, VP, VP, VP, VP]
    lh.lh_batch_read_ids.argtypes = [VP, u32p]
    lh.lh_batch_set_sampler.argtypes = [VP, C.POINTER(SampleParams), C.c_uint32, VP, VP]
    lh.lh_batch_sampler_ring_size.restype = C.c_uint32
    lh.lh_batch_sampler_ring_size.argtypes = [VP]
    lh.lh_batch_sampler_read.argtypes = [VP, C.c_uint32, u32p, u32p, C.POINTER(u64)]
    lh.lh_batch_decode_sample_lookup.argtypes = [VP, u32p, u32p, C.c_uint32, C.POINTER(LookupParams), u32p, VP, VP, VP, C.c_uint32]
    Vs, d, F, ctx_size, RING = 64, 128, 256, 16, 8
    ctx = VP()
    assert lh.lh_ctx_create(0, None, C.byref(ctx)) == 0, lh.lh_last_error(None)
    rng = np.random.default_rng(1)
    bufs, made = [], []

    def reg(shape, host=True):
        """a persistent f32 buffer of `shape` (rows, cols): random weights, or left to the device (a KV cache)"""
        rows, cols = shape
        arr = (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32) if host else None
        ne = (C.c_uint32 * 4)(cols, rows, 1, 1)
        out = u64()
        assert lh.lh_tensor_register(ctx, 0, 0, ne, 1, arr.ctypes.data if host else None, C.byref(out)) == 0, lh.lh_last_error(ctx)
        bufs.append(out.value)
        return out.value

    def shard_batch(l0, l1):
        layers = (Layer * 2)()
        layers[l0] = Layer(reg((1, d)), reg((d, d)), reg((d, d)), reg((d, d)), reg((d, d)), reg((1, d)), reg((F, d)), reg((d, F)), reg((F, d)))
        emb, norm, outw = (reg((Vs, d)), 0, 0) if l0 == 0 else (0, reg((1, d)), reg((Vs, d)))
        pods = (VP * 2)()
        for i in range(2):
            desc = Desc(Vs, d, 1, 2, F, ctx_size, l0, l1, emb, norm, outw, layers, reg((1, d * ctx_size), host=False), reg((1, d * ctx_size), host=False), 0)
            pod = VP()
            assert lh.lh_llama_create(ctx, C.byref(desc), C.byref(pod)) == 0, lh.lh_last_error(ctx)
            pods[i] = pod.value
        b = VP()
        assert lh.lh_batch_create(ctx, pods, 2, C.byref(b)) == 0, lh.lh_last_error(ctx)
        made.append((b, pods, layers))
        return b

    def state(b):
        assert lh.lh_batch_sampler_ring_size(b) == RING
        out = []
        for i in range(2):
            ring, rp, dr = (C.c_uint32 * RING)(), C.c_uint32(7), u64(7)
            assert lh.lh_batch_sampler_read(b, i, ring, C.byref(rp), C.byref(dr)) == 0, lh.lh_last_error(ctx)
            out.append((list(ring), rp.value, dr.value))
        return out

    toks, past = (C.c_uint32 * 2)(3, 5), (C.c_uint32 * 2)(0, 0)
    sp = SampleParams(40, 0.95, 0.8, 1.3, SEED)
    lp, _keep = lookup_params(1, 3, 1, None)
    ids_out = (C.c_uint32 * 8)()

    def refused(b):
        assert lh.lh_batch_decode_sample_lookup(b, toks, past, 4, C.byref(lp), ids_out, None, None, None, 0) == -4, "LH_EUNSUPPORTED"
        assert b"whole-model" in lh.lh_last_error(ctx)

    x_in = torch.from_numpy(rng.standard_normal((2, d)).astype(np.float32)).to("cuda")
    out1 = torch.zeros((2, d), dtype=torch.float32, device="cuda")
    out2 = torch.zeros((2, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        # ---- a first stage: lh_batch_set_sampler leaves it greedy (only the last stage samples); the refusal is the shard's all the same
        b = shard_batch(0, 1)
        assert lh.lh_batch_set(b, toks, past) == 0, lh.lh_last_error(ctx)
        assert lh.lh_batch_set_sampler(b, C.byref(sp), RING, None, None) == 0 and lh.lh_batch_sampler_ring_size(b) == 0
        assert lh.lh_batch_stage(b, None, VP(out1.data_ptr()), None, None) == 0, lh.lh_last_error(ctx)
        assert lh.lh_batch_set(b, toks, past) == 0
        refused(b)
        assert lh.lh_batch_stage(b, None, VP(out2.data_ptr()), None, None) == 0, lh.lh_last_error(ctx)
        assert lh.lh_ctx_sync(ctx) == 0
        a1, a2 = out1.cpu().numpy(), out2.cpu().numpy()
        assert np.all(np.isfinite(a1)) and np.abs(a1).max() > 0 and a1.tobytes() == a2.tobytes()
        # ---- a last stage: it samples
        b = shard_batch(1, 2)
        runs = []
        for disturb in (False, True):
            assert lh.lh_batch_set(b, None, past) == 0, lh.lh_last_error(ctx)
            assert lh.lh_batch_set_sampler(b, C.byref(sp), RING, None, None) == 0, lh.lh_last_error(ctx)
            fresh = state(b)
            assert fresh == [([0] * RING, 0, 0)] * 2
            if disturb:
                refused(b)
                assert state(b) == fresh, "rings, ring_pos and draws behind the refusal"
            assert lh.lh_batch_stage(b, VP(x_in.data_ptr()), None, None, None) == 0, lh.lh_last_error(ctx)
            ids = (C.c_uint32 * 2)()
            assert lh.lh_batch_read_ids(b, ids) == 0, lh.lh_last_error(ctx)
            runs.append((list(ids), state(b)))
        assert runs[0] == runs[1], "the next tick"
        for i, t in enumerate(runs[0][0]):
            assert t < Vs and runs[0][1][i] == ([t] + [0] * (RING - 1), 1, 1)
    finally:
        for b, pods, _ in made:
            lh.lh_batch_destroy(b)
            for i in range(2):
                lh.lh_llama_destroy(pods[i])
        for bf in bufs:
            lh.lh_buf_free(ctx, bf)
        lh.lh_ctx_destroy(ctx)


# ---- 10. without captured graphs ----------------------------------------------------------------------------------------------------------------
def test_without_captured_graphs_the_loop_gives_the_same_run(product, pool, monkeypatch):
    ctx, n, K, pods = 256, 33, 3, 2
    prompts = short_prompts(pods, 8)
    smp = dict(SMP, seed=SEED)
    past = [len(p) for p in prompts]
    runs = []
    for no_graph in (False, True):
        if no_graph:
            monkeypatch.setenv("LLAMAHIP_NO_GRAPH", "1")
        model = product.NewSyntheticModel(solo.make_hparams(**HD128, ctx=ctx), solo.SEED) if no_graph else pool.model("hd128", ctx, False)
        b = Batch(model, ctx, pods)
        first = start(b, prompts, ctx, smp)
        (ids, lg, stats, traces), tr = route_trace(lambda: b.DecodeSampleLookup(first, past, n - 1, K, 3, 1, None, want_logits=True))
        runs.append((first, ids, lg.tobytes(), stats, traces, [b.SamplerState(i) for i in range(pods)], b.Tick()))
        launches = [e for e in tr if e.startswith("k_sample")]
        b.free()
        if no_graph:
            model.free()
            assert launches == [f"k_sample_small_pod_rows/n{pods * (K + 1)}"] * max(st["passes"] for st in stats), launches
    assert runs[0] == runs[1] and all(st["rows"] == K + 1 for st in runs[0][3])
