"""-m gpu: jobs join and leave a SAMPLING batch (lh_batch_feed_sample), and all pods of a sampled tick in one sampler launch (k_sample_pods /
k_sample_small_pods, lh_sample_pods; k_feed_ring keeps the fed pods' lastNTokens rings).

The device sampler's uniforms are counter-based: the id of a sampling call is a function of the logits row, the ring at that moment and the call's
index.  Every check on ids is therefore an integer equality against the rule of include/llamahip.h as tests/feed_sample_ref.py restates it:
 1. op level: one multi-pod launch == the checker's llamago_SampleDebug per pod - pod counts x vocabularies x both kernels x rings that differ per pod
    (empty, partly filled, wrapped, one slot) x draws that differ per pod x logits kinds with exact ties; the rings behind the ids;
 2. a sampled tick draws the same ids with one launch as with one launch per pod (LLAMAHIP_SAMPLE_PER_POD=1), and launches what it says;
 3. NEW + prompt, then ticks == the solo sampled loop (SampleDecode of the product and of the checker) where the pass's rows are bit-identical to solo rows;
 4. a job joins a running sampled batch: the others draw what they draw undisturbed, the new job's ring really restarted;
 5. large passes: the ids are the checker's sampler on the product's OWN last-row logits (no near-tie risk), the logits within the feed's tolerance;
 6. a context swap behind a sampled feed;
 7. every refusal leaves the batch - sampler state included - as it was."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feed_sample_ref as fr       # noqa: E402
import sample_lookup_cases as sc   # noqa: E402
from test_gpu_batch import TOL, make_prompts, rel   # noqa: E402
from test_gpu_batch_feed import FEED_LENGTHS, MIXED, feed_config   # noqa: E402
from llama_go_amd.mlapi import FEED_NEW, FEED_PENDING, SHAPES, Batch, MLError, SamplePods, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu

SMP = dict(sc.SMP, repeatPenalty=1.3)   # (a penalty that moves ids: the rings matter)
SEED = 77


@pytest.fixture(scope="module")
def octx(oracle):
    return oracle.NewContext(1)


def checker_sampler(oracle, octx, seed=SEED, **kw):
    """sample(logits, ring members, draw) -> id: the checker's llamago_SampleDebug"""
    return lambda logits, members, draw: oracle.SampleTopPTopK(octx, logits, members, seed=seed, draw=draw, debug=True, **dict(SMP, **kw))[0]


# ---- 1. op level ----------------------------------------------------------------------------------------------------------------------------
KINDS = ("normal", "ties", "flat", "neginf", "zeros")
POD_COUNTS = (1, 2, 5, 64)


def pods_case(rng, V, n, rs, kind):
    """n logits rows of one kind; per pod a ring of rs slots at its own fill (empty, partly filled, full, wrapped) whose ids come mostly from the row's top
    places, where the penalty changes the answer; per pod its own draw."""
    lg = np.stack([sc.logits_of(rng, V, kind) for _ in range(n)])
    rings, pos = [], []
    for i in range(n):
        hot = np.argsort(-lg[i], kind="stable")[:4]
        cnt = (0, rs // 2, rs, 3 * rs + 2, 1)[(i + rs) % 5]
        ids = [int(hot[rng.integers(0, len(hot))]) if rng.random() < 0.7 else int(rng.integers(0, V)) for _ in range(cnt)]
        ring, p = sc.ring_after(ids, rs)
        rings.append(ring)
        pos.append(p)
    return lg, rings, pos, [int(d) for d in rng.integers(0, 1 << 40, n)]


def check_pods(product, oracle, octx, lg, rings, pos, draws, **kw):
    ids, rout, pout = SamplePods(product, lg, rings, pos, draws, seed=SEED, **dict(SMP, **kw))
    sample = checker_sampler(oracle, octx, **kw)
    for i in range(len(lg)):
        pod = fr.Pod(len(rings[i]), rings[i], pos[i], draws[i])
        want = fr.sample_step(pod, sample, lg[i])
        assert int(ids[i]) == want, (i, int(ids[i]), want, rings[i], pos[i], draws[i])
        assert [int(t) for t in rout[i]] == pod.ring and int(pout[i]) == pod.ring_pos, (i, "the ring behind the id")
    return [int(t) for t in ids]


@pytest.mark.parametrize("V", [1, 63, 1000, 1025, 32000, 40000])
def test_pods_launch_equals_the_checker_per_pod(product, oracle, octx, V):
    """Both kernels (topK 40 | 100), topK >= V where the device limit of 1024 allows it, the 4-byte load path (V % 4 != 0: rows behind the first are not
    16-byte aligned), every pod count, every ring size with every kind.  V = 40000 (> 32768): the 64-elements-per-thread instantiations of both kernels,
    two pods each."""
    rng = np.random.default_rng(V)
    case = 0
    for topK in sorted({min(40, V), min(100, V), min(V, 1024)} if V != 40000 else {40, 100}):
        for n in (POD_COUNTS if V != 40000 else (2,)):
            if V == 32000 and n == 64 and topK != 40:
                continue                                            # (64 x 32000 on the checker: once is enough)
            rs, kind = (1, 7, 64)[case % 3], KINDS[(case // 3 + case) % len(KINDS)]
            case += 1
            lg, rings, pos, draws = pods_case(rng, V, n, rs, kind)
            check_pods(product, oracle, octx, lg, rings, pos, draws, topK=topK)


@pytest.mark.parametrize("topK,topP", [(1, 0.95), (65, 0.01)])     # the deterministic settings of both kernels
def test_pods_see_their_own_rings(product, oracle, octx, topK, topP):
    """t is the maximum by a small margin, u the runner-up; whether a pod answers t or u is decided by ITS ring alone.  An empty ring (ring_pos = 0) is
    ring_size zeros: token 0 is a member.  Exact ties: value descending, then id ascending."""
    V, t, u = 1000, 700, 5
    row = np.full(V, -30.0, np.float32)
    row[t], row[u] = 10.0, 9.9
    row0 = row.copy()
    row0[0], row0[t] = 10.0, -30.0                                 # token 0 the maximum
    tie = np.full(V, -30.0, np.float32)
    tie[[900, 17, 400]] = 8.0                                      # three equal maxima: the lowest id that is not penalised wins
    lg = np.stack([row, row, row, row, row0, row0, tie, tie])
    rings = [[30, 31, 32, 33], [30, t, 32, 33], [t, 31, 32, 33], [30, 31, 32, t], [0, 0, 0, 0], [30, 31, 32, 33], [30, 31, 32, 33], [17, 31, 32, 33]]
    pos = [4, 6, 4, 8, 0, 4, 4, 5]
    got = check_pods(product, oracle, octx, lg, rings, pos, [3, 0, 9, 1, 0, 2, 5, 7], topK=topK, topP=topP, temp=1.0, repeatPenalty=1.5)
    assert got == [t, u, u, u, u, 0, 17, 400]
    # one slot per pod
    got = check_pods(product, oracle, octx, lg[:3], [[30], [t], [t]], [0, 1, 9], [0, 1, 2], topK=topK, topP=topP, temp=1.0, repeatPenalty=1.5)
    assert got == [t, u, u]


def test_sample_pods_refusals(product):
    V = 1000
    lg = np.zeros((2, V), np.float32)
    ok = dict(SMP)
    assert len(SamplePods(product, lg, [[1, 2], [3, 4]], [2, 0], [0, 1], **ok)[0]) == 2
    with pytest.raises(MLError, match="pods"):
        SamplePods(product, np.zeros((0, V), np.float32), [], [], [], **ok)
    with pytest.raises(MLError, match="pods"):
        SamplePods(product, np.zeros((65, V), np.float32), [[1]] * 65, [0] * 65, [0] * 65, **ok)
    with pytest.raises(MLError, match="vocabulary"):
        SamplePods(product, np.zeros((1, 65537), np.float32), [[1]], [0], [0], **ok)
    with pytest.raises(MLError, match="slot"):
        SamplePods(product, lg, [[], []], [0, 0], [0, 0], **ok)
    for bad, msg in ((dict(topK=0), "topK"), (dict(topK=V + 1), "topK"), (dict(temp=0.0), "temp"), (dict(repeatPenalty=0.0), "repeatPenalty")):
        with pytest.raises(MLError, match=msg):
            SamplePods(product, lg, [[1], [2]], [0, 0], [0, 0], **dict(ok, **bad))
    with pytest.raises(MLError, match="device limit"):
        SamplePods(product, np.zeros((1, 4000), np.float32), [[1]], [0], [0], **dict(ok, topK=2000))
    f = product.lib.llamago_SamplePods
    u32p, f32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    two, dr, out = (C.c_uint32 * 2)(0, 1), (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 64)()
    args = [lg.ctypes.data_as(f32p), 2, V, C.cast(two, u32p), 1, C.cast(two, u32p), C.cast(dr, u64p), 40, 0.95, 0.8, 1.1, 1, C.cast(out, u32p), None, None]
    assert f(*args) == 0
    for i in (0, 3, 5, 6, 12):
        a = list(args)
        a[i] = None
        assert f(*a) != 0 and b"null" in product.lib.ml_LastError(), i


# ---- models and solo runs, made once --------------------------------------------------------------------------------------------------------
class Pool:
    def __init__(self, product, oracle):
        self.product, self.oracle, self.models = product, oracle, {}

    def model(self, hp, seed, int8):
        key = (hp.vocabSize, hp.embdSize, hp.multSize, hp.headsCount, hp.layersCount, seed, int8)
        if key not in self.models:
            m = self.product.NewSyntheticModel(hp, seed)
            if int8:
                m.QuantizeQ8()
            self.models[key] = m
        return self.models[key]

    def solo(self, hp, mseed, int8, ctx, prompt, n, keep=0, checker=True, **smp):
        """SampleDecode of the product, equal to the checker's"""
        c = self.model(hp, mseed, int8).NewContext(ctx, 1)
        c.SetKeepCount(keep)
        run = c.SampleDecode(prompt, n, **smp)
        c.free()
        if checker:
            om = self.oracle.NewSyntheticModel(hp, mseed)
            if int8:
                om.QuantizeQ8()
            oc = om.NewContext(ctx, 16)
            oc.SetKeepCount(keep)
            orun = oc.SampleDecode(prompt, n, **smp)
            oc.free()
            om.free()
            assert run == orun, "the product's SampleDecode and the checker's"
        return run

    def close(self):
        for m in self.models.values():
            m.free()


@pytest.fixture(scope="module")
def pool(product, oracle):
    p = Pool(product, oracle)
    yield p
    p.close()


def ticks(b, ids, n):
    for _ in range(n):
        for i, t in enumerate(b.Tick()):
            ids[i].append(t)


# ---- 2. one launch per tick == one launch per pod ---------------------------------------------------------------------------------------------
TICKS = 6


def sampler_entries(trace):
    return [e for e in trace if e.startswith("k_sample")]


def tick_run(model, ctx, prompts, topK, per_pod, monkeypatch, flip_at=None):
    """a greedy feed, the sampler armed behind it, TICKS ticks -> (ids per tick, the sampler launches of every tick)"""
    if per_pod:
        monkeypatch.setenv("LLAMAHIP_SAMPLE_PER_POD", "1")
    else:
        monkeypatch.delenv("LLAMAHIP_SAMPLE_PER_POD", raising=False)
    b = Batch(model, ctx, len(prompts))
    b.Feed(prompts, [0] * len(prompts))
    b.SetSampler(seed=SEED, ringSize=ctx, **dict(SMP, topK=topK))
    ids, traces = [], []
    for t in range(TICKS):
        if t == flip_at:
            monkeypatch.setenv("LLAMAHIP_SAMPLE_PER_POD", "0" if per_pod else "1")
        got, tr = route_trace(b.Tick)
        ids.append(got)
        traces.append(sampler_entries(tr))
    b.free()
    monkeypatch.delenv("LLAMAHIP_SAMPLE_PER_POD", raising=False)
    return ids, traces


@pytest.mark.parametrize("topK", [40, 100])
@pytest.mark.parametrize("pods", [5, 9])
def test_tick_draws_the_same_ids_with_one_launch(product, pods, topK, monkeypatch):
    ctx = 32
    hp = make_hparams(**SHAPES["small"], ctx=ctx)
    prompts = make_prompts(np.random.default_rng(pods), hp.vocabSize, [1 + (i % 4) for i in range(pods)])
    one, per = ("k_sample_small_pods", "k_sample_small") if topK <= 64 else ("k_sample_pods", "k_sample")
    m = product.NewSyntheticModel(hp, 4321)
    want, tr_per = tick_run(m, ctx, prompts, topK, True, monkeypatch)
    got, tr_one = tick_run(m, ctx, prompts, topK, False, monkeypatch)
    assert got == want
    assert len({tuple(r) for r in want}) > 1, "the ticks draw ids"
    # captured ticks: the first tick runs eagerly, the second is the capture, the others replay it
    assert tr_one[:2] == [[f"{one}/n{pods}"]] * 2 and tr_per[:2] == [[per] * pods] * 2, (tr_one, tr_per)
    # the switch flipped mid-stream drops the captured tick: same ids, the other launches from there on
    for per_pod in (False, True):
        got, tr = tick_run(m, ctx, prompts, topK, per_pod, monkeypatch, flip_at=3)
        assert got == want
        a, c = ([per] * pods, [f"{one}/n{pods}"]) if per_pod else ([f"{one}/n{pods}"], [per] * pods)
        assert tr[0] == a and tr[3] == c, tr
    m.free()
    # without captured graphs every tick shows its launches: exactly one, or one per pod
    monkeypatch.setenv("LLAMAHIP_NO_GRAPH", "1")
    m = product.NewSyntheticModel(hp, 4321)
    got_per, tr_per = tick_run(m, ctx, prompts, topK, True, monkeypatch)
    got_one, tr_one = tick_run(m, ctx, prompts, topK, False, monkeypatch)
    m.free()
    assert got_per == want and got_one == want
    assert tr_one == [[f"{one}/n{pods}"]] * TICKS and tr_per == [[per] * pods] * TICKS, (tr_one, tr_per)


# ---- 3. equality with the solo loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8,lengths", [(False, [3, 1, 4]), (True, [2, 1, 1])], ids=["f32", "q8"])
def test_new_prompts_then_ticks_equal_the_solo_loop(pool, int8, lengths):
    """All pods fed NEW in one call (8 rows fp32 / 4 rows block-int8: bit-identical to solo rows), then 5 ticks: every pod's 6 ids == SampleDecode."""
    ctx, n = 64, 6
    hp = make_hparams(**dict(SHAPES["7B"], layers=2), ctx=ctx)
    prompts = make_prompts(np.random.default_rng(sum(lengths)), hp.vocabSize, lengths)
    smp = dict(SMP, seed=SEED)
    b = Batch(pool.model(hp, 4321, int8), ctx, len(prompts))
    assert b.batched
    b.SetSampler(ringSize=ctx, **smp)
    first, tr = route_trace(lambda: b.FeedSample(prompts, [0] * len(prompts), [FEED_NEW] * len(prompts)))
    assert [e for e in tr if e.startswith(("feed_pass/", "k_sample"))] == [f"feed_pass/batched/n{sum(lengths)}", f"k_sample_small_pods/n{len(prompts)}"], tr
    ids = [[i] for i in first]
    ticks(b, ids, n - 1)
    b.free()
    for i, pr in enumerate(prompts):
        assert ids[i] == pool.solo(hp, 4321, int8, ctx, pr, n, **smp), i


# ---- 4. a job joins -------------------------------------------------------------------------------------------------------------------------
def test_a_job_joins_a_running_sampled_batch(pool, oracle, octx):
    """Pods 0 and 2 draw what they draw undisturbed while pod 1 takes a new job; pod 1 then equals the solo loop of its new prompt.  topK = 1 with a
    strong penalty makes the answer a function of the ring alone: pod 1's OLD job was the one-token prompt [g], g = the id the new prompt's last row
    favours - a ring that did not restart would still hold g and answer otherwise (the rule on the product's own logits tells)."""
    ctx = 64
    hp = make_hparams(**dict(SHAPES["7B"], layers=2), ctx=ctx)
    model = pool.model(hp, 4321, False)
    p0, q, p2 = make_prompts(np.random.default_rng(4), hp.vocabSize, [3, 4, 2])
    for smp in (dict(SMP, seed=SEED), dict(SMP, seed=SEED, topK=1, repeatPenalty=1.5)):
        g = pool.solo(hp, 4321, False, ctx, q, 1, checker=False, **smp)[0]
        b = Batch(model, ctx, 3)
        b.SetSampler(ringSize=ctx, **smp)
        ids = [[i] for i in b.FeedSample([p0, [g], p2], [0, 0, 0], [FEED_NEW] * 3)]
        ticks(b, ids, 2)
        old = fr.Pod(ctx)
        fr.feed_ring(old, [g] + ids[1], FEED_NEW)                              # pod 1's ring now: its prompt and the three ids it drew
        joined, lg = b.FeedSample([[], q, []], [0, 0, 0], [0, FEED_NEW, 0], want_logits=True)
        assert joined[0] is None and joined[2] is None and np.all(np.isnan(lg[0])) and np.all(np.isnan(lg[2]))
        new = [joined[1]]
        for _ in range(3):
            t = b.Tick()
            ids[0].append(t[0])
            new.append(t[1])
            ids[2].append(t[2])
        b.free()
        assert ids[0] == pool.solo(hp, 4321, False, ctx, p0, 6, **smp) and ids[2] == pool.solo(hp, 4321, False, ctx, p2, 6, **smp)
        assert new == pool.solo(hp, 4321, False, ctx, q, 4, **smp)
        if smp.get("topK") == 1:
            assert new[0] == g
            sample = checker_sampler(oracle, octx, **{k: v for k, v in smp.items() if k != "seed"})
            kept = fr.feed(old.copy(), q, 0, sample, lg[1])                     # the same feed without the restart
            fresh = fr.feed(old.copy(), q, FEED_NEW, sample, lg[1])
            assert fresh == g and kept != g, (fresh, kept, g)


# ---- 5. large passes ------------------------------------------------------------------------------------------------------------------------
def large_cases():
    out = []
    for int8 in (False, True):
        for total in (17, 49, 65):
            out.append(pytest.param(total, int8, id=f"total{total}-{'q8' if int8 else 'f32'}"))
        out.append(pytest.param("mixed", int8, id=f"mixed-{'q8' if int8 else 'f32'}"))
    return out


@pytest.mark.parametrize("total,int8", large_cases())
def test_large_passes_sample_their_own_logits(pool, oracle, octx, total, int8):
    """Beyond the bit-identical row counts the logits are the checker's within the feed's tolerance, and the ids are EXACTLY the sampler's on the logits
    the product itself produced - over the ring the rule states: zeros + prompt at draw 0, then + the first id at draw 1 (a PENDING feed of every pod's
    pending id).  The mixed case has a solo pass (130 rows) next to a batched one."""
    if total == "mixed":
        ctx, seed = MIXED["ctx"], MIXED["seed"]
        hp = make_hparams(**SHAPES["small"], ctx=ctx)
        prompts = make_prompts(np.random.default_rng(130 + int(int8)), hp.vocabSize, MIXED["lengths"])
        passes = ["feed_pass/batched/n8", "k_sample_small_pods/n2", "feed_pass/solo/n130", "k_sample_small_pods/n1"]
    else:
        kw, prompts, seed = feed_config(total, int8)
        ctx = 64
        hp = make_hparams(**kw, ctx=ctx)
        # the schedule's rule on FEED_LENGTHS: the rows in pod order, cut at 64; a one-row remainder is a solo pass; a pod is sampled behind the pass its last row is in
        ends = np.cumsum(FEED_LENGTHS[total])
        assert int(ends[-1]) == total and total - 64 <= 1
        first = int(np.sum(ends <= 64))
        passes = [f"feed_pass/batched/n{min(total, 64)}", f"k_sample_small_pods/n{first}"]
        if total > 64:
            passes += [f"feed_pass/solo/n{total - 64}", f"k_sample_small_pods/n{len(ends) - first}"]
    B = len(prompts)
    sample = checker_sampler(oracle, octx)
    b = Batch(pool.model(hp, seed, int8), ctx, B)
    b.SetSampler(seed=SEED, ringSize=ctx, **SMP)
    (ids0, lg0), tr = route_trace(lambda: b.FeedSample(prompts, [0] * B, [FEED_NEW] * B, want_logits=True))
    launches = [e for e in tr if e.startswith(("feed_pass/", "k_sample"))]
    if not int8 or total == "mixed":
        assert launches == passes, tr
    # (block-int8 passes beyond its batched row counts run segment by segment.)  Whatever the schedule: at most one sampler launch per pass, every pod once
    assert "k_sample_small_pods/k_sample_small_pods" not in "/".join(e.split("/")[0] for e in launches) and launches[0].startswith("feed_pass/"), launches
    assert sum(int(e.rsplit("/n", 1)[1]) for e in launches if e.startswith("k_sample")) == B, launches
    ids1, lg1 = b.FeedSample([[t] for t in ids0], [len(p) for p in prompts], [FEED_PENDING] * B, want_logits=True)
    b.free()
    om = oracle.NewSyntheticModel(hp, seed)
    if int8:
        om.QuantizeQ8()
    for i, pr in enumerate(prompts):
        pod = fr.Pod(ctx, ring=[5] * ctx, ring_pos=9, draw=4)
        assert ids0[i] == fr.feed(pod, pr, FEED_NEW, sample, lg0[i]), (i, "draw 0")
        assert ids1[i] == fr.feed(pod, [ids0[i]], FEED_PENDING, sample, lg1[i]), (i, "draw 1")
        oc = om.NewContext(ctx, 16, False)
        e0, e1 = rel(lg0[i], oc.Eval(pr, 0)), rel(lg1[i], oc.Eval([ids0[i]], len(pr)))
        oc.free()
        print(f"feed_sample {total} int8 {int8} pod {i}: logits rel {e0:.2e} / {e1:.2e}")
        assert e0 <= TOL and e1 <= TOL, i
    om.free()


# ---- 6. a context swap behind a sampled feed ------------------------------------------------------------------------------------------------
def test_context_swap_behind_a_sampled_feed(pool):
    ctx, keep, n = 16, 2, 30
    hp = make_hparams(**dict(SHAPES["7B"], layers=2), ctx=ctx)
    prompts = make_prompts(np.random.default_rng(6), hp.vocabSize, [3, 1, 4])
    smp = dict(SMP, seed=SEED)
    b = Batch(pool.model(hp, 4321, False), ctx, 3)
    b.SetKeepCount(keep)
    b.SetSampler(ringSize=ctx, **smp)
    ids = [[i] for i in b.FeedSample(prompts, [0, 0, 0], [FEED_NEW] * 3)]
    ticks(b, ids, n - 1)                                                        # every pod crosses the window's end, at its own tick
    b.free()
    for i, pr in enumerate(prompts):
        assert ids[i] == pool.solo(hp, 4321, False, ctx, pr, n, keep=keep, **smp), i


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refused_feeds_leave_the_sampling_batch_as_it_was(product):
    ctx = 16
    hp = make_hparams(**SHAPES["tiny"], ctx=ctx)
    m = product.NewSyntheticModel(hp, 5)
    prompts = [[1, 2, 3], [4, 5], [6]]
    smp = dict(SMP, seed=SEED)

    def start():
        b = Batch(m, ctx, 3)
        b.SetSampler(ringSize=ctx, **smp)
        return b, [b.FeedSample(prompts, [0, 0, 0], [FEED_NEW] * 3)]

    twin, want = start()
    b, got = start()
    assert got == want
    def refusals(pos0, pend0):
        return [
            (([[], [7] * 14, []], [0, 3, 0], None), "exceeds the context window"),
            (([[hp.vocabSize], [], []], [4, 0, 0], None), "outside the vocabulary"),
            (([[], [], []], [0, 0, 0], None), "no row is fed"),
            (([[7], [], []], [pos0, 0, 0], [4, 0, 0]), "unknown flag"),
            (([[7], [], []], [pos0, 0, 0], [FEED_NEW | FEED_PENDING, 0, 0]), "exclude each other"),
            (([[pend0], [], []], [pos0 - 1, 0, 0], [FEED_PENDING, 0, 0]), "LH_FEED_PENDING needs"),                      # not the pod's position
            (([[(pend0 + 1) % hp.vocabSize], [], []], [pos0, 0, 0], [FEED_PENDING, 0, 0]), "LH_FEED_PENDING needs"),     # not its pending id
        ]

    for pos0 in (3, 4):                                                         # behind the feed, and behind a tick (the host's view of the pod has moved)
        for args, msg in refusals(pos0, got[-1][0]):
            with pytest.raises(MLError, match=msg):
                b.FeedSample(*args)
        got.append(b.Tick())
        want.append(twin.Tick())
    with pytest.raises(MLError, match="sampler"):
        b.Feed([[1], [], []], [6, 0, 0])                                        # llamago_BatchFeed on the sampling batch stays refused
    u32p = C.POINTER(C.c_uint32)
    pp = (u32p * 3)(None, None, None)
    nn, ps = (C.c_uint32 * 3)(0, 2, 0), (C.c_uint32 * 3)(0, 5, 0)
    assert product.lib.llamago_BatchFeedSample(b.h, pp, nn, ps, None, None, None, None) != 0 and "no token array" in product.last_error()
    for _ in range(2):
        got.append(b.Tick())
        want.append(twin.Tick())
    # ... and a good PENDING feed of one pod between ticks is the step the tick would have been for it
    pos = 3 + len(got) - 1
    one = b.FeedSample([[got[-1][0]], [], []], [pos, 0, 0], [FEED_PENDING, 0, 0])
    ref = twin.Tick()
    assert one[0] == ref[0]
    assert got == want
    b.free()
    twin.free()
    # no sampler set: the caller uses lh_batch_feed; the first feed of a fresh batch; PENDING on a fresh batch
    g = Batch(m, ctx, 3)
    with pytest.raises(MLError, match="no sampler set"):
        g.FeedSample(prompts, [0, 0, 0], [FEED_NEW] * 3)
    g.SetSampler(ringSize=ctx, **smp)
    with pytest.raises(MLError, match="must feed every row"):
        g.FeedSample([[1], [], [2]], [0, 0, 0], [FEED_NEW, 0, FEED_NEW])
    with pytest.raises(MLError, match="fresh batch"):
        g.FeedSample(prompts, [0, 0, 0], [FEED_PENDING] * 3)
    assert g.FeedSample(prompts, [0, 0, 0], [FEED_NEW] * 3) == want[0]
    # ClearSampler: greedy again - lh_batch_feed takes the batch, lh_batch_feed_sample does not
    g.ClearSampler()
    with pytest.raises(MLError, match="no sampler set"):
        g.FeedSample(prompts, [0, 0, 0], [FEED_NEW] * 3)
    greedy = Batch(m, ctx, 3)
    assert g.Feed(prompts, [0, 0, 0]) == greedy.Feed(prompts, [0, 0, 0]) and g.Tick() == greedy.Tick()
    greedy.free()
    g.free()
    m.free()


def test_feed_sample_refuses_a_batch_of_layer_shard_stages(product):
    """Stages of layers [0, 1) of a two-layer model, built through the C-ABI as tests/test_gpu_batch_feed.py builds them: LH_EUNSUPPORTED, and the tick
    behind the refusal writes the residual rows it writes without it."""
    import torch
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
    lh.lh_ctx_sync.argtypes = [VP]
    lh.lh_tensor_register.argtypes = [VP, u64, C.c_int, u32p, C.c_int, VP, C.POINTER(u64)]
    lh.lh_buf_free.argtypes = [VP, u64]
    lh.lh_llama_create.argtypes = [VP, C.POINTER(Desc), C.POINTER(VP)]
    lh.lh_llama_destroy.argtypes = [VP]
    lh.lh_batch_create.argtypes = [VP, C.POINTER(VP), C.c_uint32, C.POINTER(VP)]
    lh.lh_batch_destroy.argtypes = [VP]
    lh.lh_batch_set.argtypes = [VP, u32p, u32p]
    lh.lh_batch_stage.argtypes = [VP, VP, VP, VP, VP]
    lh.lh_batch_feed_sample.argtypes = [VP, C.POINTER(u32p), u32p, u32p, u32p, u32p, VP, VP]
    V, d, F, ctx_size = 64, 128, 256, 16
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
    emb = reg((V, d))
    pods = (VP * 2)()
    for i in range(2):
        desc = Desc(V, d, 1, 2, F, ctx_size, 0, 1, emb, 0, 0, layers, reg((1, d * ctx_size), host=False), reg((1, d * ctx_size), host=False), 0)
        pod = VP()
        assert lh.lh_llama_create(ctx, C.byref(desc), C.byref(pod)) == 0, lh.lh_last_error(ctx)
        pods[i] = pod.value
    b = VP()
    assert lh.lh_batch_create(ctx, pods, 2, C.byref(b)) == 0, lh.lh_last_error(ctx)
    toks, past = (C.c_uint32 * 2)(3, 5), (C.c_uint32 * 2)(0, 0)
    out1 = torch.zeros((2, d), dtype=torch.float32, device="cuda")
    out2 = torch.zeros((2, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        assert lh.lh_batch_set(b, toks, past) == 0, lh.lh_last_error(ctx)
        assert lh.lh_batch_stage(b, None, VP(out1.data_ptr()), None, None) == 0, lh.lh_last_error(ctx)
        assert lh.lh_batch_set(b, toks, past) == 0
        feed = [(C.c_uint32 * 2)(1, 2), (C.c_uint32 * 1)(4)]
        pp = (u32p * 2)(C.cast(feed[0], u32p), C.cast(feed[1], u32p))
        nn = (C.c_uint32 * 2)(2, 1)
        assert lh.lh_batch_feed_sample(b, pp, nn, past, None, None, None, None) == -4, "LH_EUNSUPPORTED"
        assert b"whole-model" in lh.lh_last_error(ctx)
        assert lh.lh_batch_stage(b, None, VP(out2.data_ptr()), None, None) == 0, lh.lh_last_error(ctx)
        assert lh.lh_ctx_sync(ctx) == 0
        a1, a2 = out1.cpu().numpy(), out2.cpu().numpy()
        assert np.all(np.isfinite(a1)) and np.abs(a1).max() > 0
        assert a1.tobytes() == a2.tobytes()
    finally:
        lh.lh_batch_destroy(b)
        for i in range(2):
            lh.lh_llama_destroy(pods[i])
        for bf in bufs:
            lh.lh_buf_free(ctx, bf)
        lh.lh_ctx_destroy(ctx)
