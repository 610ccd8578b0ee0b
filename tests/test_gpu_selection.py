"""-m gpu: the kernels that turn logits into token ids, held to independent references at their ties, edges and launch bounds.

Op level (inputs: tests/selection_cases.py, the same ones tests/test_selection_cases_cpu.py holds the references to each other on):
 - k_argmax_advance and k_batch_argmax through lh_argmax_rows: every row's id == the checker's rule (lowest index on ties; a NaN at index 0 wins,
   a NaN elsewhere is never taken), == the `argmax` of lh_score_rows on rows without NaN, and the two kernels agree on every row.  Rows are
   uploaded packed, so with V % 4 != 0 k_argmax_advance runs its 4-byte path;
 - k_sample<32|64> / k_sample_small<32|64> through lh_sample_top_p_top_k: candidates, kept count and token == tests/sampler_ref.py and == the
   checker, probabilities within the 4 ulps tests/test_gpu_sample.py grants for the device's f64 exp against libm's (NaN where the reference has
   NaN); the call without the debug outputs returns the same token.

Route level: a one-layer model whose logits are a chosen column of output.weight (the construction of tests/test_gpu_speculative.py's cycle
model), with columns that hold the same value in two or three rows - or nothing at all - so that the maximum is EXACTLY tied (asserted on the
logits read back).  Every route that picks a greedy id must pick the lowest: Eval + host argmax, the resident loop, batch prompt / tick / feed,
Verify (whose accepted count follows from it), DecodeLookup, Score; and along a chain of tied tokens the loops must stay equal to each other and
to the chain read off the matrix."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selection_cases as sc   # noqa: E402
from llama_go_amd.mlapi import Batch, argmax_rows, decode_greedy_resident, make_hparams, score_rows   # noqa: E402

pytestmark = pytest.mark.gpu


# ---- op level: the greedy kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", sc.ARGMAX_V)
def test_argmax_kernels_equal_the_rule_on_every_row(product, V):
    X, names, _ = sc.argmax_rows(V)
    want = np.array([sc.rule_argmax(x) for x in X], dtype=np.uint32)
    adv = argmax_rows(product, X, 0)       # k_argmax_advance, one launch per row
    bat = argmax_rows(product, X, 1)       # k_batch_argmax, one launch
    bad = [(names[i], int(want[i]), int(adv[i]), int(bat[i])) for i in range(len(names)) if not (adv[i] == want[i] == bat[i])]
    print(f"V={V}: {len(names)} rows, {len(bad)} differ (row, rule, k_argmax_advance, k_batch_argmax): {bad}")
    assert not bad
    assert np.array_equal(adv, bat)
    clean = np.array([not np.isnan(x).any() for x in X])
    got = score_rows(product, X[clean], [0] * int(clean.sum()))["argmax"]
    assert np.array_equal(got, want[clean]), [n for n, a, b in zip(np.array(names)[clean], got, want[clean]) if a != b]


def test_argmax_rows_refusals(product):
    from llama_go_amd.mlapi import MLError
    with pytest.raises(MLError, match="vocabulary"):
        argmax_rows(product, np.zeros((1, 65537), np.float32), 0)
    with pytest.raises(MLError, match="which"):
        argmax_rows(product, np.zeros((2, 8), np.float32), 2)
    assert list(argmax_rows(product, np.zeros((3, 65536), np.float32), 1)) == [0, 0, 0]


# ---- op level: the sampler ------------------------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("group", sc.GROUP_NAMES)
def test_sampler_kernels_equal_the_reference_on_every_case(product, oracle, group):
    hctx, octx = product.NewContext(1), oracle.NewContext(1)
    worst, bad = 0.0, []
    for i, c in enumerate(sc.groups()[group]):
        for draw in sc.DRAWS:
            tok, ids, probs = product.SampleTopPTopK(hctx, *c.args(), seed=sc.SEED, draw=draw, debug=True)
            rtok, rids, rprobs = sc.reference(group, i, draw)
            otok, oids, oprobs = oracle.SampleTopPTopK(octx, *c.args(), seed=sc.SEED, draw=draw, debug=True)
            plain = product.SampleTopPTopK(hctx, *c.args(), seed=sc.SEED, draw=draw)
            u = max(sc.ulps(probs, rprobs), sc.ulps(probs, oprobs)) if ids == rids == oids else np.inf
            if np.isfinite(u):
                worst = max(worst, u)
            if not (ids == rids == oids and len(ids) == len(rids) and u <= 4 and tok == rtok == otok and plain == tok):
                bad.append((repr(c), draw, f"kept {len(ids)} / {len(rids)}", f"ids equal: {ids == rids}", f"ulps {u}", f"token {tok} / {rtok} / {otok}, plain {plain}"))
    WORST[group] = worst
    print(f"{group}: {len(sc.groups()[group])} cases x {len(sc.DRAWS)} draws, worst probability difference {worst:.3f} ulps, {len(bad)} differ: {bad}")
    assert not bad


# ---- route level: exactly tied logits through every greedy route ----------------------------------------------------------------------------------
D = 512
CTX = 64
# single tied tokens: token -> the rows of its column that hold 1 (none: every logit is +-0)
TIED = {20: (0, 511),            # the row's first and last id
        21: (63, 64),            # the wave edge of k_batch_argmax, adjacent lanes of k_argmax_advance
        22: (252, 256),          # the wave edge of k_argmax_advance (four ids per thread)
        23: (255, 256, 257),
        24: (8, 9),              # one thread of k_argmax_advance
        25: (10, 11, 12),        # adjacent lanes of k_batch_argmax
        26: (3, 300, 500),       # first, a middle and the last wave of k_argmax_advance... and of neither mapping the same lane
        27: (3, 1),              # (listed out of order on purpose: the lowest id, not the first written)
        28: (448, 511),          # the last wave of k_batch_argmax (threads 448..511 are wave 7 of 8 that hold anything at V = 512)
        29: ()}
# a chain: the greedy successor of each token is the next one, and every step is a tie whose other members (zero columns: they lead to 0, and 0
# stays 0) are larger ids.  Closed into a cycle so that 24 steps stay on it.
CHAIN = (40, 63, 100, 252, 7, 300, 30, 128)
PARTNERS = {40: (64,), 63: (101, 511), 100: (256,), 252: (8, 9), 7: (301,), 300: (31, 448), 30: (129, 130), 128: (41,)}   # keyed by the token whose column it is; the successor joins below


def chain_rows(i):
    """the rows that tie in the column of CHAIN[i]: its successor and the partners"""
    t = CHAIN[i]
    return (CHAIN[(i + 1) % len(CHAIN)],) + PARTNERS[t]


class Tied:
    def __init__(self, product):
        hp = make_hparams(vocab=D, embd=D, mult=128, heads=4, layers=1, ctx=CTX)
        m = product.NewSyntheticModel(hp, 7)
        out = np.zeros((D, D), dtype=np.float32)
        for t, rows in TIED.items():
            out[list(rows), t] = 1
        for i, t in enumerate(CHAIN):
            rows = chain_rows(i)
            assert min(rows) == rows[0] and all(r not in CHAIN and r not in TIED for r in rows[1:])
            out[list(rows), t] = 1
        m.SetTensor("tok_embeddings.weight", np.eye(D, dtype=np.float32))
        m.SetTensor("layers.0.attention_norm.weight", np.ones(D))
        m.SetTensor("layers.0.ffn_norm.weight", np.ones(D))
        m.SetTensor("layers.0.attention.wo.weight", np.zeros((D, D)))
        m.SetTensor("layers.0.feed_forward.w2.weight", np.zeros((D, m.ffSize)))
        m.SetTensor("norm.weight", np.ones(D))
        m.SetTensor("output.weight", out)
        self.m, self.out, self.product = m, out, product

    def succ(self, t):
        """the greedy successor of t, read off the matrix with the rule (the logits are the column times one positive factor)"""
        return sc.rule_argmax(self.out[:, t])


@pytest.fixture(scope="module")
def tied(product):
    t = Tied(product)
    yield t
    t.m.free()


def test_tied_logits_are_bit_equal_and_eval_plus_host_argmax_takes_the_lowest(tied):
    """The precondition of everything below, and the first route: llama.Eval + the host argmax (GreedyContinue)."""
    c = tied.m.NewContext(CTX, 1)
    for t, rows in list(TIED.items()) + [(CHAIN[i], chain_rows(i)) for i in range(len(CHAIN))]:
        lg = c.Eval([t], 0)
        bits = lg.view(np.uint32)
        if rows:
            assert len({int(bits[r]) for r in rows}) == 1 and lg[rows[0]] > 0, (t, rows)
            others = np.delete(lg, list(rows))
            assert np.all(others < lg[rows[0]]) and np.all(others == 0), t
        else:
            assert np.all(lg == 0), t
        want = min(rows) if rows else 0
        assert tied.succ(t) == want
        assert c.GreedyContinue(t, 0, 1) == [want], (t, rows)
    c.free()


def test_every_greedy_route_takes_the_lowest_tied_id(tied):
    m = tied.m
    toks = sorted(TIED) + list(CHAIN)
    want = {t: tied.succ(t) for t in toks}
    c = m.NewContext(CTX, 1)
    for t in toks:
        assert decode_greedy_resident(c, t, 0, 1)[0] == [want[t]], ("resident loop", t)          # k_argmax_advance behind the decode kernels
        ids, a, _ = c.Verify([t], 0)
        assert (ids, a) == ([want[t]], 0), ("verify, one row", t)
        ids, _, st, _ = c.DecodeLookup(t, 0, 1, 4)
        assert ids == [want[t]], ("lookup loop", t)
        sc_row = c.Score([t], 0)
        assert int(sc_row["argmax"][0]) == want[t] and int(sc_row["target_rank"][0]) == 0, ("score", t)
    # Score of many rows at once, each against the partner that must NOT be the greedy id: rank = the number of tied ids below it
    rows = c.Score(toks, 0, targets=[max(TIED[t]) if t in TIED and TIED[t] else want[t] for t in toks])
    assert [int(r) for r in rows["argmax"]] == [want[t] for t in toks]
    assert [int(r) for r in rows["target_rank"]] == [len(TIED[t]) - 1 if t in TIED and TIED[t] else 0 for t in toks]
    c.free()
    # the pods of a batch: prompt (last row's id), tick, feed - three tokens at a time, at different positions of the three caches
    b = Batch(m, CTX, 3)
    for i in range(0, len(toks), 3):
        trio = (toks[i:i + 3] + toks[:3])[:3]
        assert b.Prompt([[5, trio[0]], [trio[1]], [6, 7, trio[2]]]) == [want[t] for t in trio], ("batch prompt", trio)
        b.Set(trio, [2, 1, 3])
        assert b.Tick() == [want[t] for t in trio], ("batch tick", trio)
        assert b.Feed([[trio[0]], [], [9, trio[2]]], [3, 0, 4]) == [want[trio[0]], None, want[trio[2]]], ("batch feed", trio)
        assert b.Feed([[trio[1], trio[0]], [trio[2]], [trio[1]]], [4, 2, 6]) == [want[trio[0]], want[trio[2]], want[trio[1]]], ("batch feed, every pod", trio)
    b.free()


def test_verify_accepts_by_the_tie_rule(tied):
    """A draft that follows the rule is accepted whole; a draft that names the OTHER tied id is cut there."""
    c = tied.m.NewContext(CTX, 1)
    n = len(CHAIN)
    for i in range(n):
        run = [CHAIN[(i + k) % n] for k in range(8)]
        ids, a, _ = c.Verify(run[:5], 0)                       # pending token + four drafted successors
        assert (ids, a) == (run[1:6], 4), (i, ids, a)
        for cut in (0, 2):                                     # the tie's other member at draft position cut + 1
            wrong = list(run[:5])
            wrong[cut + 1] = chain_rows((i + cut) % n)[-1]
            ids, a, _ = c.Verify(wrong, 0)
            assert (ids, a) == (run[1:cut + 2], cut), (i, cut, ids, a)
    c.free()


def test_chain_of_tied_tokens_is_the_same_on_every_loop(tied):
    m, steps = tied.m, 24
    start = CHAIN[:3]
    want = {}
    for s in start:
        g = [tied.succ(s)]
        while len(g) < steps:
            g.append(tied.succ(g[-1]))
        want[s] = g
        assert set(g) <= set(CHAIN) and len(set(g)) == len(CHAIN)
    c = m.NewContext(CTX, 1)
    for s in start:
        assert c.GreedyContinue(s, 0, steps) == want[s], ("Eval + host argmax", s)
        assert decode_greedy_resident(c, s, 0, steps)[0] == want[s], ("resident loop", s)
        for K in (4, 7):
            ids, _, st, _ = c.DecodeLookup(s, 0, steps, K)
            assert ids == want[s] and st["rows"] == K + 1, ("lookup loop", s, K, st)
            assert st["accepted"] > 0                              # the cycle of 8 is drafted from the window: verify rows decided ties too
    c.free()
    b = Batch(m, CTX, 3)
    got = [[t] for t in b.Prompt([[s] for s in start])]
    for _ in range(steps - 1):
        for pod, t in enumerate(b.Tick()):
            got[pod].append(t)
    assert got == [want[s] for s in start]
    b.free()
