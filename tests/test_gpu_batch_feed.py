"""-m gpu: lh_batch_feed - prompts, next turns, prompt chunks and decode rows of many pods through shared weight passes - against the checker,
against the pods' solo runs and against the per-row attention kernels.

Whatever shares a pass, every stream must compute what it computes alone (the reference runs its pods as independent llama.Contexts,
server.go:88-101, 151):
 1. prompts of different lengths fed in ONE call, then ticks: ids == the checker's, last logits within 1e-4; row totals on both sides of every route
    boundary of the batched Eval, the one-row remainder, three passes with a segment cut by a pass boundary; fp32 and block-int8;
 2. a prompt fed in chunks (7 + 1 + 15) while the other pods tick in between == the checker's solo run of the whole prompt;
 3. a new job joins a running batch: the others decode what they decode undisturbed (fp32: byte-identical logits);
 4. decode rows and prompt rows in one pass;
 5. the segment attention kernels (k_attention_seg, k_attention_split_seg) are BIT-identical to the per-row kernels on the same row table
    (LLAMAHIP_FEED_ROW_ATTN flips the route in-process), blocks that straddle the softmax branches (T = 63, 64, 65 / 127, 128, 129) and a chunk boundary,
    blocks cut short by a segment end, QB = 2 / 4 / 8; up to 8 rows (fp32) every row equals a one-token Eval on a solo context byte for byte;
 6. every fed row of a probe layer inside the float64 bound of tests/attention_ref.py, regime by regime; bit-identical behind stale cache rows;
 7. a context swap after a feed knows the fed tokens;
 8. every refusal leaves the batch as it was (the batch of layer-shard stages is built through the C-ABI: the host mirror builds whole-model batches).
Seeds: tools/check_test_margins.py feed (the checker alone must clear the 2.5 x tolerance margin; a near-tie fails, it never skips)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as R   # noqa: E402
from test_gpu_batch import MARGIN, TOL, CheckerStreams, make_prompts, rel   # noqa: E402
from llama_go_amd.mlapi import SHAPES, Batch, MLError, make_hparams, route_trace   # noqa: E402

pytestmark = pytest.mark.gpu

HD128 = dict(vocab=512, embd=640, mult=128, heads=5, layers=2)    # 5 heads of 128; ff = 1792: the block-int8 and the fp32 plane routes are built for it


def seg_entries(trace):
    return [e for e in trace if e.startswith(("k_attention_seg/", "k_attention_split_seg/"))]


def row_entries(trace):
    return [e for e in trace if e.startswith(("k_attention/rows", "k_attention_split/rows"))]


# ---- 1. equals every stream alone ----------------------------------------------------------------------------------------------------------
# prompt lengths per row total: both sides of 8 | 9 (decode stream rows | MFMA stream), 16 | 17, 32 | 33, 48 | 49 (column tiles; 49: planes on k_stream_b9),
# 64 | 65 (one pass | a one-row remainder, which runs as that pod's one-row Eval), 66 (a two-row remainder), 130 (three passes, pod 1 and pod 2 cut by a
# pass boundary)
FEED_LENGTHS = {8: [3, 1, 4], 9: [3, 2, 4], 16: [5, 1, 7, 3], 17: [5, 2, 7, 3], 32: [9, 4, 12, 7], 33: [9, 5, 12, 7], 48: [13, 6, 20, 9], 49: [13, 7, 20, 9],
                64: [20, 9, 30, 5], 65: [20, 9, 30, 6], 66: [20, 9, 30, 7], 130: [40, 50, 37, 3]}
FEED_SEEDS = {(130, False): 5000}   # (total, int8) -> model seed where the default leaves the checker at a near-tie (tools/check_test_margins.py feed)
FEED_SEED = 4321
FEED_CTX, FEED_PREDICT = 64, 5


def feed_config(total, int8):
    kw = dict(SHAPES["7B"], layers=2)
    prompts = make_prompts(np.random.default_rng(total * 131 + int(int8)), kw["vocab"], FEED_LENGTHS[total])
    return kw, prompts, FEED_SEEDS.get((total, int8), FEED_SEED)


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("total", sorted(FEED_LENGTHS))
def test_feed_equals_every_stream_alone(product, oracle, total, int8):
    """Prompts fed at position 0 in ONE call, three ticks, and the last step as a feed of every pod's pending id (a one-row Eval per pod, packed into one
    pass).  A deviation from "a feed, then 5 ticks, last-tick logits": the host library's tick returns ids only (its logits stay on the device), so the
    fifth id and the logits compared with the checker come from a FEED pass of the pending ids, not from a tick - the ids of the three ticks behind the
    feed are the checker's, and the logits of ticks are held to the checker by tests/test_gpu_batch.py."""
    kw, prompts, seed = feed_config(total, int8)
    hp = make_hparams(**kw, ctx=FEED_CTX)
    m = product.NewSyntheticModel(hp, seed)
    if int8:
        m.QuantizeQ8()
    b = Batch(m, FEED_CTX, len(prompts))
    assert b.batched
    ids = [[i] for i in b.Feed(prompts, [0] * len(prompts))]
    for _ in range(FEED_PREDICT - 2):
        for i, t in enumerate(b.Tick()):
            ids[i].append(t)
    pos = [len(p) + FEED_PREDICT - 2 for p in prompts]
    last, lg = b.Feed([[s[-1]] for s in ids], pos, want_logits=True)
    for i, t in enumerate(last):
        ids[i].append(t)
    b.free()
    m.free()
    want = CheckerStreams(oracle, hp, seed, prompts, FEED_PREDICT, FEED_CTX, int8)
    print(f"feed total {total} int8 {int8}: checker margin {want.margin:.2e}, last logits rel {rel(lg, want.last):.2e}")
    assert rel(lg, want.last) <= TOL
    want.assert_ids(ids)


MIXED = dict(lengths=[130, 3, 5], ctx=160, seed=4321)


@pytest.mark.parametrize("int8", [False, True])
def test_a_long_prompt_goes_solo_next_to_short_ones(product, oracle, int8):
    """The default schedule: a pod with 130 tokens (>= 129) is an Eval on its own plan (flash attention, last row only), the short pods share a pass.
    Ids of the feed and of three ticks, and the logits behind every prompt, against the checker."""
    ctx, seed = MIXED["ctx"], MIXED["seed"]
    hp = make_hparams(**SHAPES["small"], ctx=ctx)
    prompts = make_prompts(np.random.default_rng(130 + int(int8)), hp.vocabSize, MIXED["lengths"])
    m = product.NewSyntheticModel(hp, seed)
    if int8:
        m.QuantizeQ8()
    b = Batch(m, ctx, 3)
    (first, lg), tr = route_trace(lambda: b.Feed(prompts, [0, 0, 0], want_logits=True))
    assert [e for e in tr if e.startswith("feed_pass/")] == ["feed_pass/batched/n8", "feed_pass/solo/n130"], tr
    ids = [[i] for i in first]
    for _ in range(3):
        for i, t in enumerate(b.Tick()):
            ids[i].append(t)
    b.free()
    m.free()
    CheckerStreams(oracle, hp, seed, prompts, 4, ctx, int8).assert_ids(ids)
    om = oracle.NewSyntheticModel(hp, seed)
    if int8:
        om.QuantizeQ8()
    for i, pr in enumerate(prompts):
        oc = om.NewContext(ctx, 16, False)
        assert rel(lg[i], oc.Eval(pr, 0)) <= TOL, i
        oc.free()
    om.free()


ROW_BY_ROW = dict(kw=dict(vocab=1000, embd=200, mult=8, heads=25, layers=2), lengths=[5, 1, 8, 2, 3, 1, 4, 2, 6], seed=3, ctx=40)


def test_feed_on_a_batch_that_runs_row_by_row(product, oracle):
    """Nine pods of a model whose embd is not a multiple of 32: past the eight rows of the decode stream no P-row kernel is built for the shape, the
    batch is not batched (lh_batch_batched() == 0) and every segment of a feed is an Eval on its pod's own plan - same results, more passes."""
    kw, ctx, seed = ROW_BY_ROW["kw"], ROW_BY_ROW["ctx"], ROW_BY_ROW["seed"]
    hp = make_hparams(**kw, ctx=ctx)
    prompts = make_prompts(np.random.default_rng(kw["embd"]), kw["vocab"], ROW_BY_ROW["lengths"])
    m = product.NewSyntheticModel(hp, seed)
    b = Batch(m, ctx, len(prompts))
    assert not b.batched
    (first, tr) = route_trace(lambda: b.Feed(prompts, [0] * len(prompts)))
    assert [e for e in tr if e.startswith("feed_pass/")] == [f"feed_pass/solo/n{len(p)}" for p in prompts], tr
    ids = [[i] for i in first]
    for _ in range(3):
        for i, t in enumerate(b.Tick()):
            ids[i].append(t)
    last, lg = b.Feed([[s[-1]] for s in ids], [len(p) + 3 for p in prompts], want_logits=True)
    b.free()
    m.free()
    want = CheckerStreams(oracle, hp, seed, prompts, 5, ctx)
    assert rel(lg, want.last) <= TOL
    want.assert_ids([s + [t] for s, t in zip(ids, last)])


# ---- 2. chunks and turns -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8,seed", [(False, 4321), (True, 4321)])
def test_prompt_fed_in_chunks_while_the_others_tick(product, oracle, int8, seed):
    """Pod 1's 23-token prompt arrives as 7 + 1 + 15 tokens in three feeds; pods 0 and 2 tick in between (the ticks also advance pod 1 from its chunk's
    greedy id - the next chunk is fed at the position the prompt continues at and overwrites that row).  Pod 1 == the checker's run of the whole prompt,
    pods 0 and 2 == their undisturbed runs."""
    ctx = 48
    hp = make_hparams(**SHAPES["small"], ctx=ctx)
    rng = np.random.default_rng(23 + int(int8))
    p0, p1, p2 = make_prompts(rng, hp.vocabSize, [5, 23, 2])
    m = product.NewSyntheticModel(hp, seed)
    if int8:
        m.QuantizeQ8()
    b = Batch(m, ctx, 3)
    got = [[], [], []]

    def note(ids, pods):
        for i in pods:
            got[i].append(ids[i])

    note(b.Feed([p0, p1[:7], p2], [0, 0, 0]), (0, 2))
    for _ in range(2):
        note(b.Tick(), (0, 2))
    b.Feed([[], p1[7:8], []], [0, 7, 0])
    note(b.Tick(), (0, 2))
    ids, lg = b.Feed([[], p1[8:], []], [0, 8, 0], want_logits=True)
    note(ids, (1,))
    for _ in range(3):
        note(b.Tick(), (0, 1, 2))
    b.free()
    m.free()
    want = CheckerStreams(oracle, hp, seed, [p0, p2], 7, ctx, int8)
    want1 = CheckerStreams(oracle, hp, seed, [p1], 4, ctx, int8)
    want.assert_ids([got[0], got[2]])
    want1.assert_ids([got[1]])
    om = oracle.NewSyntheticModel(hp, seed)
    if int8:
        om.QuantizeQ8()
    oc = om.NewContext(ctx, 16, False)
    first = oc.Eval(p1, 0)
    oc.free()
    om.free()
    assert rel(lg[1], first) <= TOL          # the logits behind the last chunk = the checker's behind the whole prompt
    assert np.all(np.isnan(lg[0])) and np.all(np.isnan(lg[2])), "rows of pods that were not fed are not written"


# ---- 3. a job joins a running batch ------------------------------------------------------------------------------------------------------------
def final_step(b, ids, pos):
    """the last step as a feed of every pod's pending id: its ids and the [pods][vocab] logits"""
    return b.Feed([[t] for t in ids], pos, want_logits=True)


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("after_set", [False, True])
def test_a_job_joins_a_running_batch(product, oracle, int8, after_set):
    """Six pods, 3 ticks, then pod 2 gets a new 9-token prompt at position 0, then 3 ticks.  Pod 2 == the checker from its new prompt; the other five give
    the ids of an undisturbed run of 6 ticks, and (fp32: six rows ride the decode stream, bit-identical to solo) the logits of a last step behind them are
    byte-identical.  after_set: the feed stands between lh_batch_set and the first tick (ids_dev is stale there, tok_dev is the truth)."""
    ctx, seed = 40, 17
    hp = make_hparams(**SHAPES["small"], ctx=ctx)
    rng = np.random.default_rng(3)
    prompts = make_prompts(rng, hp.vocabSize, [5, 1, 8, 2, 12, 3])
    newp = make_prompts(rng, hp.vocabSize, [9])[0]
    lens = [len(p) for p in prompts]
    m = product.NewSyntheticModel(hp, seed)
    if int8:
        m.QuantizeQ8()
    # after_set: the ticks start from tokens of the caller's choice, NOT the ids the prompts' feed left in ids_dev (so a feed that took an unfed row's
    # next token from ids_dev instead of tok_dev would show)
    # undisturbed: prompts, (after_set: the same lh_batch_set,) 6 ticks, a last step
    b = Batch(m, ctx, 6)
    ref = [[i] for i in b.Feed(prompts, [0] * 6)]
    other = [(r[0] + 1) % hp.vocabSize for r in ref]
    if after_set:
        b.Set(other, lens)
        ref = [[o] for o in other]
    for _ in range(6):
        for i, t in enumerate(b.Tick()):
            ref[i].append(t)
    ref_last, ref_lg = final_step(b, [s[-1] for s in ref], [n + 6 for n in lens])
    b.free()
    # disturbed
    b = Batch(m, ctx, 6)
    got = [[i] for i in b.Feed(prompts, [0] * 6)]
    pre = 0 if after_set else 3
    for _ in range(pre):
        for i, t in enumerate(b.Tick()):
            got[i].append(t)
    if after_set:
        b.Set(other, lens)
        got = [[o] for o in other]
    fed = b.Feed([[], [], newp, [], [], []], [0] * 6)
    assert fed[:2] + fed[3:] == [None] * 5
    got[2] = [fed[2]]
    for _ in range(6 - pre):
        for i, t in enumerate(b.Tick()):
            got[i].append(t)
    pos = [n + 6 for n in lens]
    pos[2] = 9 + 6 - pre
    last, lg = final_step(b, [s[-1] for s in got], pos)
    b.free()
    m.free()
    for i in (0, 1, 3, 4, 5):
        assert got[i] == ref[i], i
        assert last[i] == ref_last[i]
        if not int8:
            assert lg[i].tobytes() == ref_lg[i].tobytes(), i
        else:
            assert rel(lg[i], ref_lg[i]) <= TOL
    want = CheckerStreams(oracle, hp, seed, [newp], 8 - pre, ctx, int8)
    want.assert_ids([got[2] + [last[2]]])
    assert rel(lg[2], want.last[0]) <= TOL
    if not after_set:
        CheckerStreams(oracle, hp, seed, prompts[:2], 8, ctx, int8).assert_ids([ref[0] + [ref_last[0]], ref[1] + [ref_last[1]]])
    elif not int8:
        # the chosen tokens against a solo run (six fp32 rows ride the decode stream: bit-identical to solo steps, so the ids are those of the solo run)
        m = product.NewSyntheticModel(hp, seed)
        for i in (0, 4):
            c = m.NewContext(ctx, 1)
            c.Eval(prompts[i], 0)
            tok, solo = other[i], [other[i]]
            for s_ in range(7):
                tok = int(np.argmax(c.Eval([tok], lens[i] + s_)))
                solo.append(tok)
            c.free()
            assert solo == got[i] + [last[i]], i
        m.free()


# ---- 4. decode rows and prompt rows in one pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True])
def test_decode_rows_and_prompt_rows_in_one_pass(product, oracle, int8):
    ctx, seed = 40, 17
    hp = make_hparams(**SHAPES["small"], ctx=ctx)
    rng = np.random.default_rng(44)
    prompts = make_prompts(rng, hp.vocabSize, [6, 3, 4, 2])
    new1, new3 = make_prompts(rng, hp.vocabSize, [12, 5])
    m = product.NewSyntheticModel(hp, seed)
    if int8:
        m.QuantizeQ8()
    b = Batch(m, ctx, 4)
    got = [[i] for i in b.Feed(prompts, [0] * 4)]
    for _ in range(2):
        for i, t in enumerate(b.Tick()):
            got[i].append(t)
    # pod 0: its pending id at its position (a decode row); pods 1 and 3: new prompts; pod 2 is not fed
    (fed, lg), tr = route_trace(lambda: b.Feed([[got[0][-1]], new1, [], new3], [6 + 2, 0, 0, 0], want_logits=True))
    assert [e for e in tr if e.startswith("feed_pass/")] == ["feed_pass/batched/n18"], tr
    assert fed[2] is None
    got[0].append(fed[0])
    got[1], got[3] = [fed[1]], [fed[3]]
    for _ in range(2):
        for i, t in enumerate(b.Tick()):
            got[i].append(t)
    b.free()
    m.free()
    CheckerStreams(oracle, hp, seed, [prompts[0]], 6, ctx, int8).assert_ids([got[0]])
    CheckerStreams(oracle, hp, seed, [prompts[2]], 5, ctx, int8).assert_ids([got[2]])
    w = CheckerStreams(oracle, hp, seed, [new1, new3], 3, ctx, int8)
    w.assert_ids([got[1], got[3]])
    om = oracle.NewSyntheticModel(hp, seed)
    if int8:
        om.QuantizeQ8()
    for i, pr in ((1, new1), (3, new3)):
        oc = om.NewContext(ctx, 16, False)
        assert rel(lg[i], oc.Eval(pr, 0)) <= TOL
        oc.free()
    om.free()


# ---- 5. bit-identity of the segment kernels --------------------------------------------------------------------------------------------------------
# per QB: where pod 0 / pod 1 stand before the second feed and how many rows it brings: pod 0's first block holds the rows with T = 63, 64, 65 (QB = 2:
# T = 64, 65 - the boundary between the one-wave and the two-wave softmax), pod 1's T = 127, 128, 129 (128 | 129: the softmax branch AND the chunk
# boundary of the split kernel); both segments end with a block cut short.  Pod 2: a decode row.  Pod 3: a block behind a long cache (T > 128: the
# block-wide softmax of the single pass / three chunks of the split kernel).
SEG_LAYOUT = {8: ((58, 12), (122, 10)), 4: ((61, 6), (125, 6)), 2: ((63, 3), (127, 3))}


def run_seg_feeds(m, ctx, qb, vocab, monkeypatch, row_attn):
    monkeypatch.setenv("LLAMAHIP_FEED_QB", str(qb))
    monkeypatch.setenv("LLAMAHIP_FEED_ROW_ATTN", "1" if row_attn else "0")
    (s0, n0), (s1, n1) = SEG_LAYOUT[qb]
    s3 = 200 if ctx == 256 else 300
    rng = np.random.default_rng(qb)
    toks = make_prompts(rng, vocab, [s0 + n0, s1 + n1, 4, s3 + 9])
    b = Batch(m, ctx, 4)
    try:
        assert b.batched
        out = []
        for feed in ([toks[0][:s0], toks[1][:s1], toks[2][:3], toks[3][:s3]], [toks[0][s0:], toks[1][s1:], toks[2][3:], toks[3][s3:]]):
            past = [0, 0, 0, 0] if not out else [s0, s1, 3, s3]
            (ids, last, rows), tr = route_trace(lambda: b.Feed(feed, past, want_logits=True, want_rows=True))
            out.append((ids, last, rows, tr))
        out.append(b.Tick())
        return out
    finally:
        b.free()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("qb", [8, 4, 2])
@pytest.mark.parametrize("ctx", [256, 384, 640])
def test_segment_attention_is_bit_identical_to_the_per_row_kernels(product, monkeypatch, ctx, qb, int8):
    hp = make_hparams(**HD128, ctx=ctx)
    m = product.NewSyntheticModel(hp, 8)
    if int8:
        m.QuantizeQ8()
    try:
        seg = run_seg_feeds(m, ctx, qb, HD128["vocab"], monkeypatch, False)
        row = run_seg_feeds(m, ctx, qb, HD128["vocab"], monkeypatch, True)
    finally:
        m.free()
    nch = (ctx + 127) // 128
    for k in (0, 1):
        ids_s, last_s, rows_s, tr_s = seg[k]
        ids_r, last_r, rows_r, tr_r = row[k]
        assert seg_entries(tr_s) and not row_entries(tr_s), tr_s
        assert row_entries(tr_r) and not seg_entries(tr_r), tr_r
        if ctx > 256:
            assert all(e.startswith("k_attention_split_seg/") and (f"/qb{qb}/" in e or "/qb1/" in e) for e in seg_entries(tr_s)), tr_s
            assert any(f"/qb{qb}/" in e for e in seg_entries(tr_s)), tr_s
            assert all(e.startswith(f"k_attention_split/rows/c{nch}/") for e in row_entries(tr_r)), tr_r
        else:
            assert all(e.startswith((f"k_attention_seg/hd128/qb{qb}/", "k_attention_seg/hd128/qb1/")) for e in seg_entries(tr_s)), tr_s
            assert any(f"/qb{qb}/" in e for e in seg_entries(tr_s)), tr_s
            assert all(e.startswith("k_attention/rows/hd128/") for e in row_entries(tr_r)), tr_r
        if k == 1:
            assert any("/qb1/" in e for e in seg_entries(tr_s)), "pod 2's decode row is a block of one: the QB = 1 instantiation"
        assert np.all(np.isfinite(rows_s))
        assert rows_s.tobytes() == rows_r.tobytes(), f"feed {k}: {np.count_nonzero(rows_s != rows_r)} logits differ between the segment and the per-row kernels"
        assert last_s.tobytes() == last_r.tobytes() and ids_s == ids_r
    assert seg[2] == row[2]
    # the second feed is ONE pass: its trace names the rows of both routes
    n2 = sum(n for _, n in SEG_LAYOUT[qb]) + 1 + 9
    assert [e for e in seg[1][3] if e.startswith("feed_pass/")] == [f"feed_pass/batched/n{n2}"], seg[1][3]


@pytest.mark.parametrize("shape,ctx", [("tiny", 32), ("small", 48)])
def test_segment_attention_other_head_sizes(product, monkeypatch, shape, ctx):
    """heads of 64 (tiny) take the strided score loop of the single-pass kernel; heads of 128 at a small window (small)"""
    hp = make_hparams(**SHAPES[shape], ctx=ctx)
    m = product.NewSyntheticModel(hp, 5)
    rng = np.random.default_rng(ctx)
    toks = make_prompts(rng, hp.vocabSize, [11, 1, 19, 6])
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("LLAMAHIP_FEED_ROW_ATTN", mode)
        b = Batch(m, ctx, 4)
        (ids, rows), tr = route_trace(lambda: b.Feed(toks, [0] * 4, want_rows=True))
        (ids2, rows2), _ = route_trace(lambda: b.Feed([t[:3] for t in toks], [len(t) for t in toks], want_rows=True))
        res[mode] = (ids, rows, ids2, rows2, tr)
        b.free()
    m.free()
    assert seg_entries(res["0"][4]) and not seg_entries(res["1"][4])
    assert res["0"][1].tobytes() == res["1"][1].tobytes() and res["0"][3].tobytes() == res["1"][3].tobytes()
    assert res["0"][0] == res["1"][0] and res["0"][2] == res["1"][2]


@pytest.mark.parametrize("ctx", [256, 384])
def test_up_to_eight_fed_rows_equal_solo_one_token_evals_bit_for_bit(product, ctx):
    """fp32, a pass of at most 8 rows rides the decode weight stream (every row bit-identical to its solo step) and the segment kernels repeat the per-row
    kernels' operations: each fed row's logits == llama.Eval of that one token on a context of its own, byte for byte."""
    hp = make_hparams(**HD128, ctx=ctx)
    m = product.NewSyntheticModel(hp, 8)
    rng = np.random.default_rng(ctx)
    first = make_prompts(rng, hp.vocabSize, [3, 1, 4])
    second = make_prompts(rng, hp.vocabSize, [2, 5, 1])
    b = Batch(m, ctx, 3)
    (_, rows1), tr1 = route_trace(lambda: b.Feed(first, [0, 0, 0], want_rows=True))
    (_, rows2), tr2 = route_trace(lambda: b.Feed(second, [3, 1, 4], want_rows=True))
    b.free()
    assert seg_entries(tr1) and seg_entries(tr2)
    r1 = r2 = 0
    for i in range(3):
        c = m.NewContext(ctx, 1)
        for j, t in enumerate(first[i] + second[i]):
            lg = c.Eval([t], j)
            if j < len(first[i]):
                got, r1 = rows1[r1], r1 + 1
            else:
                got, r2 = rows2[r2], r2 + 1
            assert np.asarray(lg, dtype=np.float32).tobytes() == got.tobytes(), (i, j)
        c.free()
    m.free()


# ---- 6. float64 bound, row by row ---------------------------------------------------------------------------------------------------------------
def probe_model(product, H, hd, a, b, wtype, emb):
    """The probe layer of tests/test_gpu_attention_bound.py as a whole one-layer model: attention_norm = ffn_norm = 1, wq = a I, wk = b I, wv = wo = I,
    w1 = w2 = w3 = 0, tok_embeddings = emb, norm = 1, output = I (vocab = d): logits = x_out / rms(x_out), x_out = x_in + attention(x_in)."""
    d = H * hd
    hp = make_hparams(vocab=d, embd=d, mult=128, heads=H, layers=1, ctx=64)
    m = product.NewSyntheticModel(hp, 7)
    eye, F = np.eye(d, dtype=np.float32), m.ffSize
    m.SetTensor("layers.0.attention_norm.weight", np.ones(d))
    m.SetTensor("layers.0.ffn_norm.weight", np.ones(d))
    m.SetTensor("layers.0.attention.wq.weight", np.float32(a) * eye)
    m.SetTensor("layers.0.attention.wk.weight", np.float32(b) * eye)
    m.SetTensor("layers.0.attention.wv.weight", eye)
    m.SetTensor("layers.0.attention.wo.weight", eye)
    for w, shape in (("w1", (F, d)), ("w3", (F, d)), ("w2", (d, F))):
        m.SetTensor(f"layers.0.feed_forward.{w}.weight", np.zeros(shape))
    m.SetTensor("norm.weight", np.ones(d))
    m.SetTensor("output.weight", eye)
    m.SetTensor("tok_embeddings.weight", emb)
    if wtype == "q8":
        m.QuantizeQ8()
    rd = lambda n: product.read(None, m.tensor(n)).astype(np.float64)   # noqa: E731
    W = dict(attn_norm=rd("layers.0.attention_norm.weight").reshape(d), wq=rd("layers.0.attention.wq.weight").reshape(d, d), wk=rd("layers.0.attention.wk.weight").reshape(d, d),
             wv=rd("layers.0.attention.wv.weight").reshape(d, d), wo=rd("layers.0.attention.wo.weight").reshape(d, d), norm=rd("norm.weight").reshape(d),
             output=rd("output.weight").reshape(d, d))
    assert np.all(rd("layers.0.ffn_norm.weight") == 1) and all(np.all(rd(f"layers.0.feed_forward.{w}.weight") == 0) for w in ("w1", "w2", "w3"))
    return m, W


TIE_NEIGHBOURHOOD = 128   # rows: the query rows that see the same number of 128-key chunks


def judge(name, y, refl, ref32, regime):
    """EVERY fed row on its own: each of its elements inside the bound (bound_ratio <= 1) and its error E (in rounding floors, attention_ref.case_error on
    that row alone) within K_SPREAD x the E of the float32 evaluation OF THE SAME ROW.
    The tie regime is the one exception to "the same row", by name: behind the tied keys every row resolves the same two scores of magnitude 120, where ONE
    float32 ulp of a score (2^-17) moves the tied probabilities by ~128 u - a row's E is therefore quantised by the luck of a single rounding, in the kernel
    and in the float32 evaluation alike (the float32 evaluation of this sequence: median 25 floors per row, 1.5 on its luckiest rows, 58..88 the worst of every
    64 rows).  Measured on tie-chunks at ctx 384: row 178 at 98.6 floors against that row's own float32 1.5 (fp32 weights), row 298 at 158.6 against 2.3
    (block-int8) - the per-row kernels give the same bits.  Rows that see the same number of key chunks resolve the same tie through the same sums, so they are
    samples of one distribution: a tie row is held to K_SPREAD x the WORST float32 E among the rows of its 128-row neighbourhood."""
    ref = dict(out=refl["out"], bound=refl["bound"], floor=refl["floor"])
    one = lambda r: {k: v[r:r + 1] for k, v in ref.items()}   # noqa: E731
    e_hip = np.array([R.case_error(y[r:r + 1], one(r)) for r in range(len(y))])
    e_32 = np.array([R.case_error(ref32[r:r + 1], one(r)) for r in range(len(y))])
    if regime == "tie":
        e_ref = np.array([e_32[(r // TIE_NEIGHBOURHOOD) * TIE_NEIGHBOURHOOD:(r // TIE_NEIGHBOURHOOD + 1) * TIE_NEIGHBOURHOOD].max() for r in range(len(y))])
    else:
        e_ref = e_32
    br = R.bound_ratio(y, ref)
    worst = int(np.argmax(e_hip / e_ref))
    print(f"{name}: error / bound {br:.4g}; worst row {worst}: E(hip) {e_hip[worst]:.2f} against {e_ref[worst]:.2f} (its own float32 E {e_32[worst]:.2f}); "
          f"call: E(hip) {e_hip.max():.2f}, E(float32) {e_32.max():.2f}")
    err = np.abs(y - ref["out"])
    bad = np.argwhere(~(err <= ref["bound"]))
    assert len(bad) == 0, f"{name}: {len(bad)} elements outside the bound, first (row, column) {bad[0]}: error {err[tuple(bad[0])]:.3e}, bound {ref['bound'][tuple(bad[0])]:.3e}; worst error / bound {br:.3g}"
    over = np.nonzero(~(e_hip <= R.K_SPREAD * e_ref))[0]
    assert len(over) == 0, f"{name}: row {over[0]}: error {e_hip[over[0]]:.1f} floors, the float32 evaluation's {e_ref[over[0]]:.1f}: more than {R.K_SPREAD} x ({len(over)} rows)"


BOUND_H, BOUND_HD = 4, 128
BOUND_REGIMES = [("onehot-first", "onehot", -R.G_STRONG, lambda T: (0,)), ("onehot-prev", "onehot", -R.G_STRONG, lambda T: (T - 2,)),
                 ("offset-plus", "offset", R.G_STRONG, lambda T: ()), ("offset-minus", "offset", -R.G_STRONG, lambda T: ()),
                 ("tie-chunks", "tie", -R.G_STRONG, lambda T: (127, 128)), ("ramp", "ramp", 60.0, lambda T: ())]


@pytest.mark.parametrize("wtype", ["f32", "q8"])
@pytest.mark.parametrize("ctx,T", [(256, 200), (384, 300)])
@pytest.mark.parametrize("spec", BOUND_REGIMES, ids=lambda s: s[0])
def test_every_fed_row_within_the_float64_bound(product, monkeypatch, spec, ctx, T, wtype):
    """Pod 1 is fed the regime's sequence (token t = row t of it) in ONE call next to two short neighbours: passes of 64 rows, its segments cut by every pass
    boundary (LLAMAHIP_FEED_SOLO_MIN lifted so that the long feed stays on the batched route).  ctx 256: k_attention_seg; ctx 384: k_attention_split_seg
    + the combine.  Then the same feed on a batch whose caches held decoy rows and then NaN rows: bit-identical."""
    name, regime, g, keys = spec
    H, hd, d = BOUND_H, BOUND_HD, BOUND_H * BOUND_HD
    DECOY, NAN = 400, 401                     # token ids of a decoy row and of a NaN row, beyond the sequence
    assert T <= DECOY < d
    case = R.Case(f"feed-ctx{ctx}-{name}", "", H, hd, 0, calls=[(T, 0)], regime=regime, g=g, keys=keys(T))
    X = case.sequence()
    emb = np.zeros((d, d), dtype=np.float32)
    emb[:T] = X
    emb[DECOY], emb[NAN] = R.decoy_rows(1, H, hd)[0], np.nan
    rows = np.arange(T)
    monkeypatch.setenv("LLAMAHIP_FEED_SOLO_MIN", "100000")
    model, W = probe_model(product, H, hd, case.a, case.b, wtype, emb)
    b = Batch(model, ctx, 3)
    b2 = Batch(model, ctx, 3)
    try:
        ref = R.reference(X, W, H, rows)
        assert R.check_regime(case, ref, rows) > 0
        refl = R.through_final_norm(ref, W)
        ref32 = R.f32_final_norm(R.f32_textbook(X, W, H, rows), W)
        feed = [list(range(5)), list(range(T)), list(range(3))]
        (_, lg), tr = route_trace(lambda: b.Feed(feed, [0, 0, 0], want_rows=True))
        want = "k_attention_split_seg/" if ctx > 256 else "k_attention_seg/hd128/"
        assert seg_entries(tr) and all(e.startswith(want) for e in seg_entries(tr)) and not row_entries(tr), tr
        assert len([e for e in tr if e.startswith("feed_pass/batched")]) == (T + 8 + 63) // 64, tr
        y = lg[5:5 + T].astype(np.float64)
        judge(case.name + " " + wtype, y, refl, ref32, regime)
        assert lg[:5].tobytes() == lg[5:10].tobytes(), "pod 0's rows = the same tokens at the same positions in pod 1, in the same pass"
        # stale cache rows: the window full of decoy rows, then of NaN rows, then the same feed
        for tok in (DECOY, NAN):
            b2.Feed([[tok] * ctx] * 3, [0, 0, 0])
        _, lg2 = b2.Feed(feed, [0, 0, 0], want_rows=True)
        assert lg2.tobytes() == lg.tobytes(), f"{case.name} {wtype}: the feed differs behind stale cache rows"
    finally:
        b.free()
        b2.free()
        model.free()


# ---- 7. context swap after a feed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8,seed", [(False, 16), (True, 13)])   # (fp32: seeds 12..15 leave the checker below the margin)
def test_context_swap_after_a_feed_knows_the_fed_tokens(product, oracle, int8, seed):
    """Prompts are fed (one of them in two chunks), then 80 ids go through a window of 32 with KeepCount 4: every swap re-feeds tokens the feed recorded."""
    ctx, keep, n_predict = 32, 4, 80
    hp = make_hparams(**SHAPES["small"], ctx=ctx)
    rng = np.random.default_rng(keep + int(int8))
    prompts = make_prompts(rng, hp.vocabSize, [7, 2, 9, 4])
    om = oracle.NewSyntheticModel(hp, seed)
    if int8:
        om.QuantizeQ8()
    want, margin = [], np.inf
    for pr in prompts:
        oc = om.NewContext(ctx, 16, False)
        oc.SetKeepCount(keep)
        ids, lg = oc.GreedyDecode(pr, n_predict)
        oc.free()
        srt = np.sort(lg, axis=-1)
        margin = min(margin, float(((srt[:, -1] - srt[:, -2]) / np.abs(lg).max(axis=-1)).min()))
        want.append(list(ids))
    om.free()
    if margin <= MARGIN:
        pytest.fail(f"the checker's own top-2 margin is {margin:.2e}: pick another seed")
    m = product.NewSyntheticModel(hp, seed)
    if int8:
        m.QuantizeQ8()
    b = Batch(m, ctx, 4)
    b.SetKeepCount(keep)
    b.Feed([prompts[0], prompts[1], prompts[2][:4], prompts[3]], [0, 0, 0, 0])
    b.Tick()
    got = [[i] for i in b.Feed(prompts, [0, 0, 0, 0])]        # every prompt again from position 0: what the first feed and the tick left is overwritten
    got[2] = [b.Feed([[], [], prompts[2][4:], []], [0, 0, 4, 0])[2]]   # ... and pod 2's tail once more as a chunk of its own
    for _ in range(n_predict - 1):
        for i, t in enumerate(b.Tick()):
            got[i].append(t)
    b.free()
    m.free()
    assert got == want


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------------
def test_refused_feeds_leave_the_batch_as_it_was(product):
    ctx = 16
    hp = make_hparams(**SHAPES["tiny"], ctx=ctx)
    m = product.NewSyntheticModel(hp, 5)
    prompts = [[1, 2, 3], [4, 5], [6]]

    def undisturbed():
        b = Batch(m, ctx, 3)
        out = [b.Feed(prompts, [0, 0, 0])] + [b.Tick() for _ in range(3)]
        b.free()
        return out

    want = undisturbed()
    bad = [
        (([[], [7] * 14, []], [0, 3, 0]), "exceeds the context window"),          # past + n > ctx
        (([[hp.vocabSize], [], []], [4, 0, 0]), "outside the vocabulary"),           # token id >= vocab
        (([[], [], []], [0, 0, 0]), "no row is fed"),                                # nothing to do
    ]
    b = Batch(m, ctx, 3)
    fresh = Batch(m, ctx, 3)
    with pytest.raises(MLError, match="must feed every row"):
        fresh.Feed([[1], [], [2]], [0, 0, 0])                                        # the first feed of a fresh batch
    with pytest.raises(MLError):
        fresh.Tick()                                                                 # (still fresh: no positions)
    fresh.free()
    got = [b.Feed(prompts, [0, 0, 0])]
    for k in range(3):
        (args, msg) = bad[k]
        with pytest.raises(MLError, match=msg):
            b.Feed(*args)
        got.append(b.Tick())
    assert got == want
    # a NULL token array with n_tokens > 0 (not expressible through Batch.Feed: straight through the binding)
    import ctypes as C
    u32p = C.POINTER(C.c_uint32)
    pp = (u32p * 3)(None, None, None)
    nn, ps = (C.c_uint32 * 3)(0, 2, 0), (C.c_uint32 * 3)(0, 5, 0)
    assert product.lib.llamago_BatchFeed(b.h, pp, nn, ps, None, None, None) != 0 and "no token array" in product.last_error()
    b.free()
    # after the NULL-array refusal a batch goes on as the undisturbed one does
    b = Batch(m, ctx, 3)
    got = [b.Feed(prompts, [0, 0, 0]), b.Tick()]
    assert product.lib.llamago_BatchFeed(b.h, pp, nn, ps, None, None, None) != 0
    got += [b.Tick(), b.Tick()]
    b.free()
    assert got == want
    # a batch with a sampler set: refused, and the sampled ticks behind the refusal draw what they draw without it (same seed, same state)
    drawn = []
    for refused in (False, True):
        b = Batch(m, ctx, 3)
        b.Feed(prompts, [0, 0, 0])
        b.Tick()
        b.SetSampler(seed=3)
        if refused:
            with pytest.raises(MLError, match="sampler"):
                b.Feed([[1], [], []], [4, 0, 0])
        drawn.append([b.Tick() for _ in range(3)])
        b.free()
    assert drawn[0] == drawn[1]
    m.free()


def test_feed_refuses_a_batch_of_layer_shard_stages(product):
    """A batch of layer-shard stages (here: layers [0, 1) of a two-layer model, built through the C-ABI as the cgo shim builds its stages - the host mirror
    only builds whole-model batches) is refused with LH_EUNSUPPORTED before anything is enqueued: the tick behind the refused call writes the residual rows
    it writes without it."""
    import ctypes as C
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
    lh.lh_batch_feed.argtypes = [VP, C.POINTER(u32p), u32p, u32p, u32p, VP, VP]
    V, d, F, ctx_size = 64, 128, 256, 16
    ctx = VP()
    assert lh.lh_ctx_create(0, None, C.byref(ctx)) == 0, lh.lh_last_error(None)
    rng = np.random.default_rng(1)
    bufs = []

    def reg(shape, host=True):
        """a persistent f32 buffer of `shape` (rows, cols): random weights, or left to the device (a KV cache)"""
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
        assert lh.lh_batch_feed(b, pp, nn, past, None, None, None) == -4, "LH_EUNSUPPORTED"
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
