"""not-gpu: tests/feed_sample_ref.py (the rule of lh_batch_feed_sample, which the GPU tests hold the device to) against the checker.
 - NEW + prompt, then sampling steps, keeps the ring the bookkeeping of the checker's llama_SampleDecode keeps (oracle.c: ring_size zeros, the prompt
   appended, sample s as call s over the whole ring, the id appended), the ids from llamago_SampleDebug(seed, draw); ring sizes below and above the prompt;
 - a PENDING feed of the pod's own pending id is a plain step; a feed without flags appends every token; a NEW feed forgets the old job;
 - on a model: the rule over the checker's own Evals draws what its SampleDecode draws;
 - the entry points are declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feed_sample_ref as fr
import sample_lookup_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMP = dict(sc.SMP, repeatPenalty=1.3)


@pytest.fixture(scope="module")
def checker(built):
    from llama_go_amd.mlapi import MLLib
    lib = MLLib(os.path.join(ROOT, "oracle", "liboracle.so"))
    return lib, lib.NewContext(1)


def sampler(checker, seed, **kw):
    lib, ctx = checker
    return lambda logits, members, draw: lib.SampleTopPTopK(ctx, logits, members, seed=seed, draw=draw, debug=True, **dict(SMP, **kw))[0]


def bookkeeping(sample, prompt, rows, ring_size):
    """oracle.c llama_SampleDecode, the Evals replaced by given logits rows -> (ids, the ring after every step)."""
    ring, pos, ids, rings = [0] * ring_size, 0, [], []
    for t in prompt:
        ring[pos % ring_size] = t
        pos += 1
    for s, lg in enumerate(rows):
        tok = int(sample(lg, list(ring), s))
        ring[pos % ring_size] = tok
        pos += 1
        ids.append(tok)
        rings.append((tuple(ring), pos, s + 1))
    return ids, rings


@pytest.mark.parametrize("ring_size", [1, 3, 8, 64])
def test_new_prompt_then_steps_keeps_the_checkers_ring(checker, ring_size):
    V = 300
    rng = np.random.default_rng(ring_size)
    below = above = 0
    for case in range(6):
        n_prompt = (1, 2, 4, 7, 9, 12)[case]
        below, above = below + (ring_size < n_prompt), above + (ring_size > n_prompt)
        rows = [sc.logits_of(rng, V, "normal") for _ in range(5)]
        hot = np.argsort(-rows[0])[:3]
        prompt = [int(hot[i % 3]) if i % 2 else int(rng.integers(0, V)) for i in range(n_prompt)]   # ids whose penalty changes the answer
        sample = sampler(checker, seed=case)
        want_ids, want_rings = bookkeeping(sample, prompt, rows, ring_size)
        pod = fr.Pod(ring_size, ring=rng.integers(0, V, ring_size), ring_pos=int(rng.integers(0, 100)), draw=int(rng.integers(0, 100)))   # an old job's state
        got = [fr.feed(pod, prompt, fr.FEED_NEW, sample, rows[0])]
        assert pod.key() == want_rings[0]
        for s in (1, 2):                                                  # ticks
            got.append(fr.sample_step(pod, sample, rows[s]))
            assert pod.key() == want_rings[s]
        for s in (3, 4):                                                  # the same steps as feeds of the pod's own pending id
            got.append(fr.feed(pod, [got[-1]], fr.FEED_PENDING, sample, rows[s]))
            assert pod.key() == want_rings[s]
        assert got == want_ids
    assert ring_size >= 64 or below, "a ring below the prompt length was among the cases"
    assert ring_size <= 1 or above, "a ring above the prompt length was among the cases"


def test_next_turn_without_flags_and_pending_with_more_tokens(checker):
    V, rs = 200, 5
    rng = np.random.default_rng(1)
    sample = sampler(checker, seed=3)
    rows = [sc.logits_of(rng, V, "normal") for _ in range(3)]
    pod = fr.Pod(rs)
    a = fr.feed(pod, [7, 8], fr.FEED_NEW, sample, rows[0])
    assert pod.key() == ((7, 8, a, 0, 0), 3, 1)
    turn = pod.copy()
    b = fr.feed(turn, [9, 10, 11], 0, sample, rows[1])                   # a next turn: every token appended behind the pending id's slot
    assert turn.key() == ((11, b, a, 9, 10), 7, 2)
    pend = pod.copy()
    c = fr.feed(pend, [a, 9, 10], fr.FEED_PENDING, sample, rows[1])      # the pending id first: it is in the ring already
    assert pend.key() == ((c, 8, a, 9, 10), 6, 2)
    with pytest.raises(AssertionError):
        fr.feed(pod, [1], fr.FEED_NEW | fr.FEED_PENDING, sample, rows[2])


def test_a_new_job_forgets_the_old_ring(checker):
    """The old ring holds the new prompt's favourite id, a restarted one does not: with topK = 1 the answers differ."""
    V, t, u = 100, 60, 5
    row = np.full(V, -30.0, np.float32)
    row[t], row[u] = 10.0, 9.9
    sample = sampler(checker, seed=1, topK=1, repeatPenalty=1.5)
    old = fr.Pod(8, ring=[t] * 8, ring_pos=11, draw=4)
    kept, fresh = old.copy(), old.copy()
    assert fr.feed(kept, [20, 21], 0, sample, row) == u
    assert fr.feed(fresh, [20, 21], fr.FEED_NEW, sample, row) == t
    assert fresh.key() == ((20, 21, t, 0, 0, 0, 0, 0), 3, 1)


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "q8"])
def test_rule_over_the_checkers_evals_equals_its_sample_decode(checker, int8):
    from llama_go_amd.mlapi import SHAPES, make_hparams
    lib, _ = checker
    ctx, n, seed = 24, 6, 11
    m = lib.NewSyntheticModel(make_hparams(**SHAPES["tiny"], ctx=ctx), sc.MODEL_SEED)
    if int8:
        m.QuantizeQ8()
    prompt = sc.prompt_for(SHAPES["tiny"]["vocab"], 5)
    c = m.NewContext(ctx, 4)
    want = c.SampleDecode(prompt, n, seed=seed, **SMP)
    c.free()
    c = m.NewContext(ctx, 4)
    sample = sampler(checker, seed=seed)
    pod = fr.Pod(ctx, ring=[9] * ctx, ring_pos=3, draw=2)
    got = [fr.feed(pod, prompt, fr.FEED_NEW, sample, c.Eval(prompt, 0))]
    for s in range(1, n):
        lg = c.Eval([got[-1]], len(prompt) + s - 1)
        got.append(fr.sample_step(pod, sample, lg) if s % 2 else fr.feed(pod, [got[-1]], fr.FEED_PENDING, sample, lg))
    c.free()
    m.free()
    assert got == want


def test_entry_points_are_declared_exported_and_bound(built):
    import llama_go_amd as pkg
    from llama_go_amd import mlapi
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)   # noqa: E731
    raw = open(os.path.join(ROOT, "include", "llamahip.h")).read()
    hip_hdr, ext_hdr = strip(raw), strip(open(os.path.join(ROOT, "include", "llamago_ext.h")).read())
    hip, go = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL), C.CDLL(pkg.LIBLLAMAGO)
    for n in ("lh_batch_feed_sample", "lh_sample_pods"):
        assert re.search(r"\b" + n + r"\s*\(", hip_hdr) and hasattr(hip, n), n
    for n in ("llamago_BatchFeedSample", "llamago_SamplePods"):
        assert re.search(r"\b" + n + r"\s*\(", ext_hdr) and hasattr(go, n), n
    assert re.search(r"enum\s*\{\s*LH_FEED_NEW\s*=\s*1\s*,\s*LH_FEED_PENDING\s*=\s*2\s*\}", hip_hdr)
    assert (mlapi.FEED_NEW, mlapi.FEED_PENDING) == (fr.FEED_NEW, fr.FEED_PENDING) == (1, 2)
    assert hasattr(mlapi.Batch, "FeedSample") and hasattr(mlapi, "SamplePods")
    shim = open(os.path.join(ROOT, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    assert re.search(r"\bC\.lh_batch_feed_sample\s*\(", shim) and "FeedSample" in shim
    for phrase in ("LH_FEED_PENDING the first one is NOT appended", "ONE feed", "LLAMAHIP_SAMPLE_PER_POD"):
        assert phrase in raw, phrase
    hip.lh_batch_feed_sample.restype = hip.lh_sample_pods.restype = C.c_int
    assert hip.lh_batch_feed_sample(None, None, None, None, None, None, None, None) == -1     # LH_EINVAL
    assert hip.lh_sample_pods(None, None, 1, 8, None, 1, None, None, None, None, None, None) == -1
