"""-m gpu: lossless lookup-draft speculative decoding (lh_draft_lookup, lh_llama_verify, lh_llama_decode_lookup; kernels_spec.h).

The claim is exactness, so every check is an equality:
 1. the device drafter == the rule of tests/speculative_ref.py on random windows (alphabets that make matches at every n-gram length), window
    lengths 1 / G / G + 1 / ctx, with and without a corpus, unknown entries, every limit;
 2. a verify pass with a forced draft accepts exactly the prefix the model itself produces (full, cut at the first / a middle / the last entry, cut
    where the wrong entry is a valid LATER continuation), leaves a state from which the resident greedy loop yields the rest of the undisturbed run
    (fp32: last logits byte for byte), also behind stale and NaN cache rows; single-pass (ctx 256) and split (ctx 384) attention; block-int8;
 3. the loop == lh_llama_decode_greedy: ids, fp32 last logits byte for byte, stats and per-pass trace == the simulation, the state left behind;
 4. the same across two context swaps;
 5. the 32-layer synthetic 7B against the committed golden ids with the pinned pass counts;
 6. every refusal leaves the context as it was.
Every loop test asserts stats.rows == draft_max + 1: a silent fall-back to plain steps fails."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speculative_ref as ref   # noqa: E402
from llama_go_amd.mlapi import PROMPT, SHAPES, MLError, decode_greedy_resident, draft_lookup, make_hparams   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD128 = dict(vocab=512, embd=640, mult=128, heads=5, layers=2)    # tests/test_gpu_batch_feed.py: 5 heads of 128, both weight types' row kernels are built for it
U = ref.UNKNOWN
NAN_TOKEN = 511                                                   # its embedding row is NaN in the "hd128nan" models below: what poisons stale cache rows
SEED = 4321


def kmax(int8):
    return 3 if int8 else 7


# ---- models and undisturbed greedy runs, made once ------------------------------------------------------------------------------------------
class Pool:
    def __init__(self, product):
        self.product, self.models, self.runs = product, {}, {}

    def model(self, name, ctx, int8):
        key = (name, ctx, int8)
        if key not in self.models:
            kw = HD128 if name.startswith("hd128") else dict(SHAPES["7B"], layers=2)
            m = self.product.NewSyntheticModel(make_hparams(**kw, ctx=ctx), SEED)
            if name == "hd128nan":   # the same weights, one token's embedding NaN (the verify tests poison stale cache rows with it)
                emb = self.product.read(None, m.tensor("tok_embeddings.weight")).reshape(kw["vocab"], kw["embd"]).copy()
                emb[NAN_TOKEN] = np.nan
                m.SetTensor("tok_embeddings.weight", emb)
            if int8:
                m.QuantizeQ8()
            self.models[key] = m
        return self.models[key]

    def greedy(self, name, ctx, int8, prompt, n, keep=0):
        """(ids g[0..n), last logits, logits of one more Eval behind the run) of prompt -> n greedy ids: g[0] = argmax behind the prompt, the rest
        from the resident loop."""
        key = (name, ctx, int8, tuple(prompt), n, keep)
        if key not in self.runs:
            c = self.model(name, ctx, int8).NewContext(ctx, 1)
            c.SetKeepCount(keep)
            first = int(np.argmax(c.Eval(prompt, 0)))
            toks, lg = decode_greedy_resident(c, first, len(prompt), n - 1, want_logits=True)
            more = c.Eval([toks[-1]], len(prompt) + n - 1) if len(prompt) + n - 1 < ctx else None
            c.free()
            g = [first] + toks
            assert NAN_TOKEN not in g or name != "hd128nan", "the greedy run produced the NaN token: choose another prompt for this test"
            self.runs[key] = (g, lg, more)
        return self.runs[key]

    def close(self):
        for m in self.models.values():
            m.free()


@pytest.fixture(scope="module")
def pool(product):
    p = Pool(product)
    yield p
    p.close()


def prompt_for(vocab, n, seed=7):
    return [int(t) for t in np.random.default_rng(seed).integers(0, min(vocab, NAN_TOKEN), n)]


# ---- 1. the drafter against the Python rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", [3, 8, 512])
def test_draft_lookup_equals_the_python_rule(product, alphabet):
    rng = np.random.default_rng(alphabet)
    ctx, checked, nonempty = 256, 0, 0
    for gmax, gmin in ((3, 1), (8, 1), (4, 4), (2, 2), (1, 1)):
        for n in sorted({1, gmax, gmax + 1, 2 * gmax + 3, ctx}):
            for corpus_len in (0, 1, gmax + 1, 300):
                for unknown in (False, True):
                    win = [int(t) for t in rng.integers(0, alphabet, n)]
                    corpus = [int(t) for t in rng.integers(0, alphabet, corpus_len)] or None
                    if unknown and n > 2:
                        for i in rng.integers(0, n, max(1, n // 8)):
                            win[int(i)] = U
                    K = int(rng.integers(1, 8))
                    want = ref.draft(win, K, gmax, gmin, corpus)
                    got = draft_lookup(product, win, K, gmax, gmin, corpus)
                    assert got == want, (alphabet, gmax, gmin, n, corpus_len, unknown, K)
                    checked, nonempty = checked + 1, nonempty + bool(want)
    assert nonempty >= (checked // 4 if alphabet <= 8 else 0), (checked, nonempty)


def test_draft_lookup_limits_corpus_only_match_and_window_first(product):
    H = [1, 2, 3, 4, 5, 6, 7, 8, 1]
    for K in (1, 4, 7):
        for limit in range(0, K + 1):
            assert draft_lookup(product, H, K, 1, 1, limit=limit) == ref.draft(H, K, 1, 1, limit=limit) == [2, 3, 4, 5, 6, 7, 8][:min(K, limit)]
    assert draft_lookup(product, [8, 3, 4], 3, 2, 1, corpus=[7, 4, 5, 6]) == [5, 6]       # a corpus match only the smaller G finds
    assert draft_lookup(product, [8, 3, 4], 3, 2, 2, corpus=[7, 4, 5, 6]) == []
    assert draft_lookup(product, [1, 4, 9, 1], 7, 1, 1, corpus=[1, 6, 7]) == [4, 9, 1]    # the window is searched first
    assert draft_lookup(product, [9, 1], 7, 1, 1, corpus=[5, 6, 1]) == []                 # a match at the corpus' last token has no continuation
    assert draft_lookup(product, [4, 4, 4], 4, 2, 2) == [4]                               # the suffix may not match itself
    assert draft_lookup(product, [3, 8, U, 6, 3], 4, 1, 1) == [8]                         # the draft ends in front of an unknown entry
    big = [int(t) for t in np.random.default_rng(1).integers(0, 4, 65536)]                # the corpus cap, more than one stride of the block
    win = [int(t) for t in np.random.default_rng(2).integers(0, 4, 2048)]
    assert draft_lookup(product, [U] * 9 + win[-8:], 7, 8, 1, corpus=big) == ref.draft([U] * 9 + win[-8:], 7, 8, 1, corpus=big)
    assert draft_lookup(product, win, 7, 8, 1, corpus=big) == ref.draft(win, 7, 8, 1, corpus=big)


# ---- 2. verify with forced drafts -------------------------------------------------------------------------------------------------------------
N_RUN = 16   # ids of the undisturbed run: g[0] pending behind the prompt, up to 7 drafted, the rest decoded from the state verify leaves


def fresh_context(model, ctx, prompt, stale):
    c = model.NewContext(ctx, 1)
    if stale:   # the cache held a longer run of other tokens, then NaN rows, behind the prompt
        c.Eval(prompt_for(HD128["vocab"], 40, seed=99), 0)
        c.Eval([NAN_TOKEN] * 48, 0)
    c.Eval(prompt, 0)
    return c


@pytest.mark.parametrize("stale", [False, True], ids=["clean", "stale"])
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
@pytest.mark.parametrize("ctx", [256, 384])
def test_verify_accepts_exactly_what_the_model_produces(pool, ctx, int8, stale):
    model = pool.model("hd128nan", ctx, int8)
    prompt = prompt_for(HD128["vocab"], 8)
    g, lg_last, _ = pool.greedy("hd128nan", ctx, int8, prompt, N_RUN)
    V, past = HD128["vocab"], len(prompt)
    cases = []
    for k in ((1, 3) if int8 else (1, 3, 7)):
        cases.append((g[1:1 + k], k))                                    # the model's own continuation: accepted whole
        for j in sorted({0, k // 2, k - 1}):
            d = g[1:1 + k]
            d[j] = next(t for t in range(V) if t not in (g[1 + j], NAN_TOKEN))
            cases.append((d, j))                                         # corrupted at j: cut there
            if g[2 + j] != g[1 + j]:
                d = g[1:1 + k]
                d[j] = g[2 + j]                                          # the wrong entry is the NEXT id of the run: still cut at j
                cases.append((d, j))
    cases.append(([], 0))                                                # no draft: one row, the plain step
    for draft, want_a in cases:
        c = fresh_context(model, ctx, prompt, stale)
        ids, a, lg = c.Verify([g[0]] + draft, past, want_logits=True)
        assert a == want_a and ids == g[1:a + 2], (draft, want_a, a, ids, g)
        assert int(np.argmax(lg)) == ids[-1]
        rest, lg2 = decode_greedy_resident(c, ids[-1], past + a + 1, N_RUN - 2 - a, want_logits=True)
        assert rest == g[a + 2:], (draft, rest, g)
        if not int8:
            assert lg2.tobytes() == lg_last.tobytes(), (draft, "last logits of the run behind the verify pass")
        c.free()


def test_verify_on_the_7b_matrix_shapes(pool):
    ctx = 64
    model = pool.model("7b", ctx, False)
    g, lg_last, _ = pool.greedy("7b", ctx, False, PROMPT, 12)
    d = g[1:8]
    d[4] = (d[4] + 1) % 32000
    for draft, want_a in ((g[1:8], 7), (d, 4)):
        c = model.NewContext(ctx, 1)
        c.Eval(PROMPT, 0)
        ids, a, _ = c.Verify([g[0]] + draft, len(PROMPT))
        assert a == want_a and ids == g[1:a + 2]
        rest, lg2 = decode_greedy_resident(c, ids[-1], len(PROMPT) + a + 1, 12 - 2 - a, want_logits=True)
        assert rest == g[a + 2:] and lg2.tobytes() == lg_last.tobytes()
        c.free()


# ---- 3. the loop equals greedy ----------------------------------------------------------------------------------------------------------------
def run_lookup(pool, name, ctx, int8, prompt, n, K, corpus, keep=0, gmax=3, gmin=1, stats_exact=True):
    """DecodeLookup of n - 1 steps behind the prompt against the undisturbed greedy run of the same settings."""
    g, lg_last, more = pool.greedy(name, ctx, int8, prompt, n, keep)
    c = pool.model(name, ctx, int8).NewContext(ctx, 1)
    c.SetKeepCount(keep)
    first = int(np.argmax(c.Eval(prompt, 0)))
    assert first == g[0]
    ids, lg, st, tr = c.DecodeLookup(first, len(prompt), n - 1, K, gmax, gmin, corpus, want_logits=True)
    assert st["rows"] == K + 1, st
    assert ids == g[1:], (ids, g)
    if not int8:
        assert lg.tobytes() == lg_last.tobytes(), "last logits"
    assert st["passes"] == len(tr) <= n - 1 and all(a <= k <= K for k, a in tr) and sum(a + 1 for _, a in tr) == n - 1
    assert st["drafted"] == sum(k for k, _ in tr) and st["accepted"] == sum(a for _, a in tr) and st["empty"] == sum(1 for k, _ in tr if k == 0)
    if stats_exact:
        vocab = pool.model(name, ctx, int8).hp.vocabSize
        want_tr, want_st = ref.simulate(list(prompt) + [g[0]], g[1:], n - 1, K, gmax, gmin, corpus, ctx, vocab, keep)
        assert tr == want_tr and st == want_st, (tr, want_tr)
    if more is not None:   # the state left behind: one more Eval gives what it gives behind the greedy loop
        again = c.Eval([ids[-1]], len(prompt) + n - 1)
        assert (again.tobytes() == more.tobytes()) if not int8 else (int(np.argmax(again)) == int(np.argmax(more)))
    c.free()
    return st, tr


def cycle_model(product, ctx):
    """One layer, vocab = d, one-hot embeddings, wo = w2 = 0, norms 1, output = the matrix of a map sigma: the greedy successor of t is sigma(t).
    sigma: a 5-cycle on 10..14, one cycle of 507 over the rest."""
    d = 512
    hp = make_hparams(vocab=d, embd=d, mult=128, heads=4, layers=1, ctx=ctx)
    m = product.NewSyntheticModel(hp, 7)
    rest = list(range(10)) + list(range(15, d))
    sigma = {t: 10 + (t - 10 + 1) % 5 for t in range(10, 15)}
    sigma.update({t: rest[(i + 1) % len(rest)] for i, t in enumerate(rest)})
    out = np.zeros((d, d), dtype=np.float32)
    for t, s in sigma.items():
        out[s, t] = 1
    m.SetTensor("tok_embeddings.weight", np.eye(d, dtype=np.float32))
    m.SetTensor("layers.0.attention_norm.weight", np.ones(d))
    m.SetTensor("layers.0.ffn_norm.weight", np.ones(d))
    m.SetTensor("layers.0.attention.wo.weight", np.zeros((d, d)))
    m.SetTensor("layers.0.feed_forward.w2.weight", np.zeros((d, m.ffSize)))
    m.SetTensor("norm.weight", np.ones(d))
    m.SetTensor("output.weight", out)
    return m, sigma


def test_loop_on_a_cycle_model(product):
    ctx, n = 64, 41
    m, sigma = cycle_model(product, ctx)
    for start, K in ((10, 4), (10, 7), (20, 7)):
        prompt = [3, 4, start]
        g = [sigma[start]]
        while len(g) < n:
            g.append(sigma[g[-1]])
        c = m.NewContext(ctx, 1)
        first = int(np.argmax(c.Eval(prompt, 0)))
        ids, _, st, tr = c.DecodeLookup(first, len(prompt), n - 1, K, 3, 1)
        c.free()
        assert [first] + ids == g and st["rows"] == K + 1, (start, K, st)
        want_tr, want_st = ref.simulate(prompt + [g[0]], g[1:], n - 1, K, 3, 1, None, ctx)
        assert tr == want_tr and st == want_st, (start, K, tr, want_tr)
        if start == 10 and K == 4:      # inside the 5-cycle: behind the warm-up every pass drafts K and accepts K (the last one clipped by what remains)
            assert tr[:4] == [(0, 0)] * 4 and all(t == (4, 4) for t in tr[4:-1]) and tr[-1][0] == tr[-1][1]
        if start == 10 and K == 7:      # the largest j is one period back: the window's end cuts the continuation at 5
            assert all(t == (5, 5) for t in tr[4:])
        if start == 20:                 # a cycle longer than the run: every draft is empty
            assert st["empty"] == st["passes"] == n - 1 and st["drafted"] == 0
    m.free()


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
@pytest.mark.parametrize("ctx", [256, 384])
def test_loop_equals_greedy_on_random_weights(pool, ctx, int8):
    K, n = kmax(int8), 48
    prompt = prompt_for(HD128["vocab"], 8)
    g, _, _ = pool.greedy("hd128", ctx, int8, prompt, n)
    st, tr = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, prompt + g)                # (b) the replay corpus: every draft accepted whole
    assert st["accepted"] == st["drafted"] > 0 and st["passes"] <= (n - 1 + K) // (K + 1) + 1 and tr[-1][0] <= K
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, None)                               # (c) the window alone
    bad = list(prompt + g)
    for i in range(len(prompt) + 5, len(bad), 5):                                          # a corpus that is wrong at every fifth id: partial acceptance
        bad[i] = (bad[i] + 1) % NAN_TOKEN
    st, tr = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, bad, gmax=2)
    assert any(0 < a < k for k, a in tr) or any(a == 0 < k for k, a in tr), tr
    for steps in (2, 3, K + 2, 2 * K + 3):                                                 # (d) the last pass clipped by remaining - 1
        run_lookup(pool, "hd128", ctx, int8, prompt, steps + 1, K, prompt + g)


def test_loop_on_the_7b_matrix_shapes(pool):
    g, _, _ = pool.greedy("7b", 64, False, PROMPT, 40)
    st, _ = run_lookup(pool, "7b", 64, False, PROMPT, 40, 7, PROMPT + g)
    assert st["accepted"] == st["drafted"] > 0
    run_lookup(pool, "7b", 64, False, PROMPT, 40, 3, PROMPT + g)


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_loop_clipped_by_the_window_then_swaps(pool, int8):
    """(d) a start 13 positions in front of the window's end: the passes there shrink with what is left of the window (row counts R - 1 .. 1), then the
    context swaps as the greedy loop does and full passes go on."""
    ctx, keep, K, n = 256, 8, kmax(int8), 40
    prompt = prompt_for(HD128["vocab"], ctx - 13, seed=11)
    g, _, _ = pool.greedy("hd128", ctx, int8, prompt, n, keep)
    st, tr = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, prompt + g, keep=keep)
    assert st["accepted"] > 0
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, None, keep=keep)


# ---- 4. across context swaps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_loop_across_two_context_swaps(pool, int8):
    ctx, keep, K, n = 64, 8, kmax(int8), 101     # from position 8: the first swap after 56 ids, the second 28 later
    prompt = prompt_for(HD128["vocab"], 8)
    g, _, _ = pool.greedy("hd128", ctx, int8, prompt, n, keep)
    st, _ = run_lookup(pool, "hd128", ctx, int8, prompt, n, K, prompt + g, keep=keep, stats_exact=False)
    assert st["passes"] <= n - 1
    run_lookup(pool, "hd128", ctx, int8, prompt, n, K, None, keep=keep, stats_exact=False)


# ---- 5. full depth ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_golden_workload_at_full_depth(product, int8):
    """All 32 layers of the synthetic 7B (tests/test_gpu_llama.py::test_headline_workload_at_full_depth): ids[1:100] of the committed golden run, with
    the pass counts tests/test_speculative_ref_cpu.py pins."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "7b_seed1234_int8_ids.json" if int8 else "7b_seed1234_ids.json")))["ids"]
    K = kmax(int8)
    m = product.NewSyntheticModel(make_hparams(**SHAPES["7B"], ctx=128), 1234)
    if int8:
        m.QuantizeQ8()
    for corpus, want in ((PROMPT + gold, (25, 74, 74) if int8 else (13, 86, 86)), (None, (98, 36, 1) if int8 else (95, 79, 4))):
        c = m.NewContext(128, 1)
        first = int(np.argmax(c.Eval(PROMPT, 0)))
        ids, _, st, tr = c.DecodeLookup(first, len(PROMPT), 99, K, 3, 1, corpus)
        c.free()
        assert [first] + ids == gold, "ids"
        assert st["rows"] == K + 1 and (st["passes"], st["drafted"], st["accepted"]) == want, st
        want_tr, want_st = ref.simulate(PROMPT + [gold[0]], gold[1:], 99, K, 3, 1, corpus, 128)
        assert tr == want_tr and st == want_st
    m.free()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_refusals_leave_the_context_as_it_was(pool, product, int8):
    ctx, n = 256, 12
    model = pool.model("hd128", ctx, int8)
    prompt = prompt_for(HD128["vocab"], 8)
    g, lg_last, _ = pool.greedy("hd128", ctx, int8, prompt, n)
    V, K, past = HD128["vocab"], kmax(int8), len(prompt)
    c = model.NewContext(ctx, 1)
    c.Eval(prompt, 0)
    bad_loops = [dict(draft_max=0), dict(draft_max=K + 1), dict(draft_max=K, ngram_min=0), dict(draft_max=K, ngram_max=2, ngram_min=3),
                 dict(draft_max=K, ngram_max=9), dict(draft_max=K, corpus=[1] * 65537), dict(draft_max=K, corpus=[1, 2, V, 3])]
    for kw in bad_loops:
        with pytest.raises(MLError):
            c.DecodeLookup(g[0], past, n - 1, **kw)
    with pytest.raises(MLError):
        c.DecodeLookup(V, past, n - 1, K)                       # a first token outside the vocabulary
    with pytest.raises(MLError, match="exceeds the context window"):
        c.Verify([g[0]] + g[1:3], ctx - 2)                      # past + n > ctx
    with pytest.raises(MLError):
        c.Verify([g[0]] * (K + 2), past)                        # more rows than the weight type carries
    with pytest.raises(MLError):
        c.Verify([g[0], V], past)                               # a draft id outside the vocabulary
    with pytest.raises(MLError):
        c.Verify([], past)
    toks, lg = decode_greedy_resident(c, g[0], past, n - 1, want_logits=True)
    assert toks == g[1:] and (int8 or lg.tobytes() == lg_last.tobytes()), "the context decodes what it would have decoded"
    c.free()
    # a layer-shard stage: refused as unsupported, by name
    hp = make_hparams(**HD128, ctx=ctx)
    shard = product.NewSyntheticModel(hp, SEED, 0, 1)
    sc = shard.NewContext(ctx, 1)
    with pytest.raises(MLError, match="whole-model"):
        sc.DecodeLookup(1, 0, 4, K)
    with pytest.raises(MLError, match="whole-model"):
        sc.Verify([1, 2], 0)
    sc.free()
    shard.free()
