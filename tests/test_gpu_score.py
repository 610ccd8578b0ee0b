"""-m gpu: scoring token sequences on the device (csrc/kernels_score.h, lh_score_rows / lh_llama_score) against numpy float64 and the checker.

Definition restated here in numpy f64 (include/llamahip.h, lh_row_score): m = max x; s = sum exp((double)x - m); lse = m + ln s;
logprob = x[t] - lse; argmax = lowest index of the maximum; target_rank = #{x_j > x_t} + #{j < t : x_j == x_t}.

Model-level margins (chosen on the CPU with the checker, tools/check_test_margins.py style): the token sequences below are
default_rng(SEQ_SEED[...]).integers(0, V, n); the checker's smallest relative top-2 margin over their rows is
  tiny fp32 4.16e-3 (row 29)   tiny int8 2.56e-3 (row 35)   7B slice fp32 1.67e-3 (row 20)   7B slice int8 1.64e-3 (row 20)      (MARGIN = 2.5e-4)
On the 7B slice the checker's n single-prefix Evals cost CPU minutes beyond 33 rows, so n stays <= 33 there.
"""
import json
import os

import numpy as np
import pytest

from llama_go_amd.mlapi import PROMPT, SHAPES, MLError, make_hparams, score_rows

pytestmark = pytest.mark.gpu
TOL = 1e-4
MARGIN = 2.5 * TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- numpy float64 restatement ------------------------------------------------------------------------------------------------------------
def ref_row(x, t):
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        m = x64.max()                                   # NaN if the row holds one
        if np.isnan(m) or np.isinf(m):
            lse = np.nan
        else:
            lse = m + np.log(np.exp(x64 - m).sum())
    xt = x[t]
    return dict(logprob=float(np.float64(xt) - lse), lse=float(lse), target_logit=xt, max_logit=np.float32(m), argmax=int(np.argmax(x)),
                target_rank=int((x > xt).sum() + (x[:t] == xt).sum()))


def f64_bound(V, lse):
    """one-ulp f64 exp and log plus the worst case V * 2^-53 of an f64 sum of V non-negative terms in any order, doubled"""
    return 4 * V * 2.0 ** -53 * max(1.0, abs(lse))


def check_rows(got, x, targets, nan_rows=()):
    V = x.shape[1]
    for i in range(x.shape[0]):
        want = ref_row(x[i], targets[i])
        g = got[i]
        if i in nan_rows or np.isnan(want["lse"]):
            assert np.isnan(g["logprob"]) and np.isnan(g["lse"]), (i, g)
            assert g["argmax"] < V
            if not np.isnan(x[i]).any():                # +inf / all -inf rows: the greedy id is still the lowest index of the maximum
                assert g["argmax"] == want["argmax"], (i, g, want)
            continue
        assert g["argmax"] == want["argmax"] and g["target_rank"] == want["target_rank"], (i, g, want)
        assert g["max_logit"] == want["max_logit"] and g["target_logit"] == want["target_logit"], (i, g, want)
        b = f64_bound(V, want["lse"])
        print(f"row {i}: V {V} lse err {abs(g['lse'] - want['lse']):.3e} logprob err {abs(g['logprob'] - want['logprob']):.3e} bound {b:.3e}")
        assert abs(g["lse"] - want["lse"]) <= b, (i, g["lse"], want["lse"], b)
        assert abs(g["logprob"] - want["logprob"]) <= b, (i, g["logprob"], want["logprob"], b)


# ---- 1. op level ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 7, 64])
@pytest.mark.parametrize("V", [512, 32000, 32001, 50000])
def test_score_rows_random_rows_match_numpy_f64(product, V, n_rows):
    rng = np.random.default_rng(V * 3 + n_rows)
    x = (rng.standard_normal((n_rows, V)) * 4).astype(np.float32)
    targets = [int(t) for t in rng.integers(0, V, n_rows)]
    targets[0] = 0
    targets[-1] = V - 1
    check_rows(score_rows(product, x, targets), x, targets)


@pytest.mark.parametrize("V", [512, 32000, 32001, 50000])
def test_score_rows_ties_infinities_and_nan(product, V):
    rng = np.random.default_rng(V + 17)
    n = 12
    x = (rng.standard_normal((n, V)) * 4).astype(np.float32)
    targets = [int(t) for t in rng.integers(0, V, n)]
    top = np.float32(np.abs(x).max() + 1)
    x[0, [V - 1, 37, V // 2]] = top                         # ties for the maximum: the lowest index (37) is the greedy id
    x[1, [3, V // 3 + 1, V - 2]] = top                      # ... in different threads / waves of the kernel's layout
    targets[1] = V - 2                                      # the target is a tie of the maximum, but not the first: rank 2
    x[2] = np.round(x[2] * 2) / 2                           # many ties everywhere, also at the target
    x[3, ::3] = x[3, 5]                                     # a third of the row equals one value
    targets[3] = 3 * (V // 6)                               # the target inside that run of ties: rank counts the equal entries before it
    x[4, rng.integers(0, V, V // 3)] = -np.inf              # -inf entries add 0
    x[5, :] = -np.inf                                       # all -inf: NaN, argmax 0
    x[6, V // 3] = np.nan                                   # a NaN: NaN, argmax < V
    x[7, [V - 5, 11]] = np.inf                              # +inf: NaN, argmax 11
    targets[8], targets[9] = 0, V - 1                       # the target at both ends
    x[10, :] = -0.75                                        # a constant row: lse = -0.75 + ln V, rank = the target's index
    x[11, 0] = top                                          # the maximum at index 0 and the target on it
    targets[11] = 0
    x[4, targets[4]] = 1.5                                  # (a finite target in the -inf row)
    got = score_rows(product, x, targets)
    check_rows(got, x, targets, nan_rows=(5, 6, 7))
    assert got[0]["argmax"] == 37 and got[1]["argmax"] == 3 and got[1]["target_rank"] == 2
    assert got[5]["argmax"] == 0 and got[7]["argmax"] == 11
    assert got[10]["target_rank"] == targets[10] and got[11]["target_rank"] == 0


def test_score_rows_rejects_targets_outside_the_vocabulary(product):
    x = np.zeros((3, 1000), np.float32)
    with pytest.raises(MLError, match="target id 1000 of row 1"):
        score_rows(product, x, [0, 1000, 5])
    with pytest.raises(MLError, match="target id"):
        score_rows(product, x, [0, 1, 0xFFFFFFFF])           # (the library's own "greedy id" marker is not part of the interface)


# ---- 2. model level, against the checker ----------------------------------------------------------------------------------------------------
CONFIGS = {   # name -> (shape, layers, int8, context, rows the checker is asked for)
    "tiny": ("tiny", None, False, 128, 65), "tiny_q8": ("tiny", None, True, 128, 65),
    "7b": ("7B", 2, False, 64, 33), "7b_q8": ("7B", 2, True, 64, 33),
}
SEQ_SEED = {"tiny": 1, "tiny_q8": 1, "7b": 2, "7b_q8": 2}   # (7B slice, seed 1: row 16 of the fp32 checker is a near-tie, 1.4e-4)
_ROWS = {}


def _hp(name):
    shape, layers, _, ctx, _ = CONFIGS[name]
    kw = dict(SHAPES[shape])
    if layers:
        kw["layers"] = layers
    return make_hparams(**kw, ctx=ctx)


def _seq(name, n=None):
    hp = _hp(name)
    s = [int(t) for t in np.random.default_rng(SEQ_SEED[name]).integers(0, hp.vocabSize, CONFIGS[name][4])]
    return s if n is None else s[:n]


def checker_rows(oracle, name):
    """row i = the checker's last-row logits of Eval(seq[:i+1], 0): it has no all-row entry.  One pass per configuration and session."""
    if name not in _ROWS:
        _, _, int8, ctx, n = CONFIGS[name]
        om = oracle.NewSyntheticModel(_hp(name), 1234)
        if int8:
            om.QuantizeQ8()
        oc = om.NewContext(ctx, 16, False)
        seq = _seq(name)
        _ROWS[name] = np.stack([oc.Eval(seq[:i + 1], 0) for i in range(n)])
        oc.free()
        om.free()
    return _ROWS[name]


def product_model(product, name):
    m = product.NewSyntheticModel(_hp(name), 1234)
    if CONFIGS[name][2]:
        m.QuantizeQ8()
    return m


def check_against_checker(got, ref_logits, row0, targets):
    """got[k] scores the logits behind token row0 + k; ref_logits = the checker's rows of the whole sequence; targets[k] None = the greedy id"""
    for k in range(len(got)):
        lo = ref_logits[row0 + k]
        s = np.sort(lo)
        margin = float((s[-1] - s[-2]) / np.abs(lo).max())
        assert margin > MARGIN, f"row {row0 + k}: the checker's own logits have a near-tie ({margin:.2e}): pick another sequence seed"
        t = int(np.argmax(lo)) if targets[k] is None else targets[k]
        want = ref_row(lo, t)
        bound = 2 * TOL * float(np.abs(lo).max())
        print(f"row {row0 + k}: logprob gpu {got[k]['logprob']:.6f} checker {want['logprob']:.6f} err {abs(got[k]['logprob'] - want['logprob']):.3e} bound {bound:.3e} margin {margin:.2e}")
        assert abs(got[k]["logprob"] - want["logprob"]) <= bound, (row0 + k, got[k], want)
        assert got[k]["argmax"] == want["argmax"], (row0 + k, got[k], want)


@pytest.mark.parametrize("name,n", [(c, n) for c in CONFIGS for n in (1, 2, 8, 9, 33, 64, 65) if n <= CONFIGS[c][4]])
def test_score_matches_checker(product, oracle, name, n):
    ref = checker_rows(oracle, name)
    seq = _seq(name, n)
    m = product_model(product, name)
    c = m.NewContext(CONFIGS[name][3], 1)
    got = c.Score(seq, 0)
    c.free()
    m.free()
    assert len(got) == n
    check_against_checker(got, ref, 0, seq[1:] + [None])
    assert got[-1]["target_rank"] == 0 and got[-1]["target_logit"] == got[-1]["max_logit"]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_score_behind_a_scored_prefix(product, oracle, name):
    """past = 17: the rows behind a prefix that was itself scored (its K/V rows are the ones the second call attends to), explicit targets"""
    ref = checker_rows(oracle, name)
    seq = _seq(name, 33)
    m = product_model(product, name)
    c = m.NewContext(CONFIGS[name][3], 1)
    a = c.Score(seq[:17], 0)
    tg = seq[18:] + [seq[0]]
    b = c.Score(seq[17:], 17, targets=tg)
    c.free()
    m.free()
    check_against_checker(a, ref, 0, seq[1:17] + [None])
    check_against_checker(b, ref, 17, tg)


def test_score_errors(product):
    m = product_model(product, "tiny")
    c = m.NewContext(32, 1)
    with pytest.raises(MLError, match="context window"):
        c.Score(list(range(20)), 13)
    with pytest.raises(MLError, match="target id"):
        c.Score([1, 2, 3], 0, targets=[1, 512, 2])
    with pytest.raises(MLError, match="token id"):
        c.Score([1, 512, 3], 0)
    with pytest.raises(MLError):
        c.Score([], 0)
    c.free()
    m.free()


# ---- 3. consistency -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_q8"])
def test_score_in_chunks_equals_one_call(product, oracle, name):
    ref = checker_rows(oracle, name)
    seq = _seq(name, 64)
    m = product_model(product, name)
    c = m.NewContext(128, 1)
    one = c.Score(seq, 0)
    for cuts in ((40,), (9, 42)):
        parts, lo = [], 0
        for hi in list(cuts) + [64]:
            parts.append(c.Score(seq[lo:hi], lo, targets=(seq[lo + 1:hi + 1] if hi < 64 else seq[lo + 1:64] + [seq[0]])))
            lo = hi
        chunked = np.concatenate(parts)
        for i in range(64):
            lo_i = ref[i]
            s = np.sort(lo_i)
            assert (s[-1] - s[-2]) / np.abs(lo_i).max() > MARGIN, f"row {i}: near-tie in the checker's logits, pick another sequence seed"
            assert chunked[i]["argmax"] == one[i]["argmax"], (cuts, i)
            if i < 63:                                  # (the last row's target differs: greedy id there, seq[0] here)
                assert abs(chunked[i]["logprob"] - one[i]["logprob"]) <= 2 * TOL * float(np.abs(lo_i).max()), (cuts, i)
    c.free()
    m.free()


@pytest.mark.parametrize("name,n_prompt", [("tiny", 8), ("tiny", 40), ("tiny_q8", 8), ("7b", 8)])
def test_decoding_continues_from_a_scored_prompt(product, name, n_prompt):
    """Score leaves the KV cache (and the context's token history) as Eval does: the greedy continuation is the same."""
    prompt = _seq(name, n_prompt)
    m = product_model(product, name)
    ctx = CONFIGS[name][3]
    c = m.NewContext(ctx, 1)
    first = int(np.argmax(c.Eval(prompt, 0)))
    want = [first] + c.GreedyContinue(first, n_prompt, 6)
    c.free()
    c = m.NewContext(ctx, 1)
    rows = c.Score(prompt, 0)
    got = [int(rows[-1]["argmax"])] + c.GreedyContinue(int(rows[-1]["argmax"]), n_prompt, 6)
    c.free()
    m.free()
    assert got == want


# ---- 4. full depth, teacher forcing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int8", [False, True])
def test_teacher_forcing_reproduces_the_golden_ids_at_full_depth(product, int8):
    """All 32 layers of the synthetic 7B: the golden prompt followed by the first 56 / 40 golden ids in ONE scored Eval - every row from the
    prompt's last on must pick the id the checker decoded step by step (min_top2_margin_rel of the file against a GPU-vs-checker error of
    6e-6: no row is excused)."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "7b_seed1234_int8_ids.json" if int8 else "7b_seed1234_ids.json")))
    assert gold["oracle_ids_match"] and gold["min_top2_margin_rel"] > TOL
    ids = gold["ids"]
    m = product.NewSyntheticModel(make_hparams(**SHAPES["7B"], ctx=128), 1234)
    if int8:
        m.QuantizeQ8()
    c = m.NewContext(128, 1)
    for n_ids in (56, 40):
        tokens = PROMPT + ids[:n_ids]
        rows = c.Score(tokens, 0)
        n = len(tokens)
        assert n == 8 + n_ids
        for i in range(7, n):
            assert rows[i]["argmax"] == ids[i - 7], (n, i, rows[i], ids[i - 7])
            assert rows[i]["target_rank"] == 0, (n, i, rows[i])          # rows with a next token: it is the greedy id; the last row: by definition
            assert np.isfinite(rows[i]["logprob"]) and rows[i]["logprob"] <= 0
    c.free()
    m.free()


# ---- 5. perplexity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_q8"])
def test_perplexity_follows_the_window_convention(product, name):
    ctx = 64
    hp = _hp(name)
    tokens = [int(t) for t in np.random.default_rng(5).integers(0, hp.vocabSize, 2 * ctx + 5)]
    m = product_model(product, name)
    c = m.NewContext(ctx, 1)
    want, terms, bound = 0.0, 0, 0.0
    for w0 in range(0, len(tokens), ctx):
        win = tokens[w0:w0 + ctx]
        rows = c.Score(win, 0)
        for i in range(len(win) - 1):                    # the window's last row is not scored
            want -= rows[i]["logprob"]
            bound += 2 * TOL * abs(float(rows[i]["max_logit"]))   # (|max logit| <= max |logit|: not wider than the row bound of the model-level tests)
            terms += 1
    assert terms == 2 * (ctx - 1) + 4
    for chunk in (0, 24, 1):
        nll, cnt = c.Perplexity(tokens, chunk)
        print(f"{name} chunk {chunk}: nll_sum {nll:.9f} rebuilt {want:.9f} diff {abs(nll - want):.3e} bound {bound:.3e} n_scored {cnt} perplexity {np.exp(nll / cnt):.4f}")
        assert cnt == terms
        assert abs(nll - want) <= bound
    assert c.Perplexity(tokens[:1]) == (0.0, 0)          # a window of one token is dropped
    c.free()
    m.free()


def test_perplexity_fp32_and_int8_on_the_7b_slice(product):
    """The first model-level figure of the block-int8 format: both finite; the two values and their ratio are PRINTED, nothing is asserted
    about the ratio (random weights: it says little about real models)."""
    hp = _hp("7b")
    tokens = [int(t) for t in np.random.default_rng(6).integers(0, hp.vocabSize, 64 + 10)]
    ppl = {}
    for name in ("7b", "7b_q8"):
        m = product_model(product, name)
        c = m.NewContext(64, 1)
        nll, cnt = c.Perplexity(tokens)
        c.free()
        m.free()
        assert cnt == 63 + 9 and np.isfinite(nll) and nll > 0
        ppl[name] = float(np.exp(nll / cnt))
    print(f"7B slice (2 layers, synthetic): perplexity fp32 {ppl['7b']:.4f} int8 {ppl['7b_q8']:.4f} ratio {ppl['7b_q8'] / ppl['7b']:.6f}")
    assert np.isfinite(ppl["7b"]) and np.isfinite(ppl["7b_q8"])
