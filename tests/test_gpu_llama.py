"""-m gpu: end-to-end parity of llama.Eval on the MI355X against the oracle, through the C-ABI.

Three executions of the same model are compared on the same seeded synthetic weights and prompts:
  oracle      CPU restatement of the reference's pure-Go arithmetic (the checker)
  hip/generic lh_graph_compute with LH_GRAPH_NO_FUSION: one kernel per ml op, reference graph order
  hip/fused   lh_graph_compute recognising the Eval graph -> fused plan (+ hipGraph replay for N = 1)

Contract (BASELINE.json north_star): logits within 1e-4 relative (max|delta| / max|ref|), greedy token ids exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

import json

from llama_go_amd.mlapi import PROMPT, SHAPES, decode_greedy_resident, make_hparams

pytestmark = pytest.mark.gpu
TOL = 1e-4
MARGIN = 2.5 * TOL   # ids are asserted only where the checker itself is not at a near-tie; a near-tie FAILS the test (pick another seed)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def greedy_margin(lg):
    s = np.sort(lg, axis=-1)
    return float(((s[..., -1] - s[..., -2]) / np.abs(lg).max(axis=-1)).min())


def decode_both(product, oracle, shape, ctx, prompt, n_predict, seed=1234, layers=None, threads=16):
    kw = dict(SHAPES[shape])
    if layers:
        kw["layers"] = layers
    hp = make_hparams(**kw, ctx=ctx)
    out = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, seed)
        c = m.NewContext(ctx, threads, False)
        out[name] = c.GreedyDecode(prompt, n_predict)
        if name == "hip":
            product.lib.llamago_LastGraphFused.restype = C.c_int
            product.lib.llamago_LastGraphFused.argtypes = [C.c_void_p]
            out["fused"] = product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h))
        c.free()
        m.free()
    return out


@pytest.mark.parametrize("kw,ctx,n_prompt", [
    (dict(vocab=300, embd=384, mult=32, heads=6, layers=2), 96, 40),      # head dim 64, ragged vocabulary, ff = 1024
    (dict(vocab=1000, embd=256, mult=16, heads=8, layers=3), 300, 70),    # head dim 32, context > 256, ff = 688 (not a tile multiple)
    (dict(vocab=515, embd=640, mult=8, heads=5, layers=2), 300, 7),       # 5 heads of 128, odd vocabulary, context > 256 (split attention)
    (dict(vocab=2048, embd=1024, mult=256, heads=8, layers=1), 40, 1),    # single-token prompt
    (dict(vocab=777, embd=512, mult=64, heads=4, layers=2), 160, 130),    # two row tiles, ragged second one
])
def test_odd_shapes_match_oracle(product, oracle, kw, ctx, n_prompt):
    """Shapes outside the LLaMA family's (head dims 32 / 64, ragged vocabularies and ff sizes, contexts on both sides of the
    split-attention threshold): prefill (whatever kernel family the shape selects) + decode steps against the checker."""
    hp = make_hparams(**kw, ctx=ctx)
    rng = np.random.default_rng(n_prompt + kw["embd"])
    prompt = [int(t) for t in rng.integers(0, kw["vocab"], n_prompt)]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 99)
        c = m.NewContext(ctx, 16, False)
        res[name] = c.GreedyDecode(prompt, 6)
        c.free()
        m.free()
    (th, lh_), (to, lo) = res["hip"], res["orc"]
    assert rel(lh_, lo) <= TOL
    assert greedy_margin(lo) > MARGIN, "the checker's own logits have a near-tie: pick another seed (tools/check_test_margins.py)"
    assert th == to


@pytest.mark.parametrize("kw,ctx,n_prompt", [
    (dict(vocab=515, embd=640, mult=32, heads=5, layers=2), 300, 7),      # odd vocabulary, 5 heads, context > 256, decode-path prefill
    (dict(vocab=300, embd=384, mult=32, heads=6, layers=2), 96, 40),      # head dim 64: per-query attention behind the int8 GEMM
    (dict(vocab=777, embd=512, mult=64, heads=4, layers=2), 200, 150),    # two row tiles, ragged second one, ragged vocabulary
])
def test_odd_shapes_block_int8(product, oracle, kw, ctx, n_prompt):
    hp = make_hparams(**kw, ctx=ctx)
    rng = np.random.default_rng(n_prompt + kw["embd"] + 1)
    prompt = [int(t) for t in rng.integers(0, kw["vocab"], n_prompt)]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 99).QuantizeQ8()
        c = m.NewContext(ctx, 16, False)
        res[name] = c.GreedyDecode(prompt, 5)
        c.free()
        m.free()
    (th, lh_), (to, lo) = res["hip"], res["orc"]
    assert rel(lh_, lo) <= TOL
    assert greedy_margin(lo) > MARGIN, "the checker's own logits have a near-tie: pick another seed (tools/check_test_margins.py)"
    assert th == to


@pytest.mark.parametrize("n_prompt", [8, 40, 60, 100, 300])
def test_results_are_bitwise_reproducible(product, n_prompt):
    """Fixed reduction orders everywhere (wave trees, split-K partials summed by a second pass, no float atomics): the same Eval
    twice, on fresh contexts, gives the same bits — for the weight-stream, 64-row-tile, split-K and multi-tile GEMM paths."""
    kw = dict(SHAPES["small"])
    kw["layers"] = 2
    hp = make_hparams(**kw, ctx=320)
    rng = np.random.default_rng(n_prompt)
    prompt = [int(t) for t in rng.integers(0, kw["vocab"], n_prompt)]
    m = product.NewSyntheticModel(hp, 1234)
    outs = []
    for _ in range(2):
        c = m.NewContext(320, 1, False)
        a = c.Eval(prompt, 0)
        b = c.Eval([3], n_prompt)
        outs.append((a, b))
        c.free()
    m.free()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_concurrent_pods_share_one_model(product):
    """The reference serves several pods at once: goroutines with their own llama.Context over ONE shared Model (server.go:45,
    88-101, 151).  Four Python threads (ctypes releases the GIL during the calls) run the generation loop concurrently on their own
    contexts and streams; every pod must produce exactly what it produces alone."""
    import threading
    kw = dict(SHAPES["small"])
    hp = make_hparams(**kw, ctx=96)
    m = product.NewSyntheticModel(hp, 1234)
    prompts = [[1, 5, 9, 200], [7, 8], [300, 2, 2, 2, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55], [11] * 40]
    alone = []
    for pr in prompts:
        c = m.NewContext(96, 1, False)
        alone.append(c.GreedyDecode(pr, 24, want_logits=False)[0])
        c.free()
    got, errs = [None] * len(prompts), []

    def pod(i):
        try:
            c = m.NewContext(96, 1, False)
            for _ in range(3):
                got[i] = c.GreedyDecode(prompts[i], 24, want_logits=False)[0]
            c.free()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ths = [threading.Thread(target=pod, args=(i,)) for i in range(len(prompts))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    m.free()
    assert not errs, errs
    assert got == alone


def test_pods_come_and_go_without_leaking_hbm(product):
    """server.Do creates a llama.Context per job and drops it (server.go:151): context create / use / release in a loop — also from
    concurrent threads, also the resident plans and pipelines — must hand every byte of device memory back (KV caches registered per
    pod are freed with the pod: the Go shim's ReleaseContextHIP, mirrored by llama_ReleaseContext here).  And the model may neither be
    re-quantised nor released under live contexts."""
    import threading
    import torch
    from llama_go_amd.mlapi import MLError, Pipeline, decode_greedy_resident
    hp = make_hparams(**SHAPES["small"], ctx=256)
    m = product.NewSyntheticModel(hp, 1234)

    def job(n_ctx=256):
        c = m.NewContext(n_ctx, 1, False)
        toks = c.GreedyDecode([1, 5, 9, 200], 4, want_logits=False)[0]
        decode_greedy_resident(c, toks[-1], 8, 3)          # resident plan + captured graph on this context
        c.SampleDecode([1, 5, 9], 3, seed=1)
        c.free()

    job()                                                   # warm-up: module load, code objects, first-use pools
    pl = Pipeline(m, 256, 2)
    pl.run([[1, 2, 3], [4]], 2)
    pl.free()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(6):
        job()
    ths = [threading.Thread(target=job) for _ in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    pl = Pipeline(m, 256, 3)
    pl.run([[1, 2, 3], [4], [5, 6]], 2)
    pl.free()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 <= 4 << 20, f"{(free0 - free1) / 2**20:.1f} MiB of HBM not returned after the pods ended"
    # live context: quantising would free the f32 weights its plans address
    c = m.NewContext(64, 1, False)
    c.Eval([1, 2], 0)
    with pytest.raises(MLError):
        m.QuantizeQ8()
    product.lib.llama_FreeModel(m.h)                        # deferred: the context still holds the model (Go: the Context keeps it reachable)
    assert int(np.argmax(c.Eval([3], 2))) >= 0              # ... and keeps working
    c.free()                                                # last user gone: the model is released now
    m.h = None
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free2 > free1


def test_chunked_prefill_all_kernel_families(product, oracle):
    """One context fed in chunks of 3, 9, 20, 40, 70 and 1 tokens: every Eval continues from a non-empty cache (past > 0) and takes a
    different kernel family (weight stream with token rows in registers, MFMA GEMM with 64-row tiles + per-query attention, MFMA
    GEMM + batched-GEMM attention with causal skipping, decode graph)."""
    kw = dict(SHAPES["small"])
    kw["layers"] = 2
    hp = make_hparams(**kw, ctx=160)
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, kw["vocab"], 143)]
    chunks = [3, 9, 20, 40, 70, 1]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 1234)
        c = m.NewContext(160, 16, False)
        out, past = [], 0
        for n in chunks:
            out.append(c.Eval(toks[past:past + n], past))
            past += n
        c.free()
        m.free()
        res[name] = out
    for a, b in zip(res["hip"], res["orc"]):
        assert rel(a, b) <= TOL


def test_two_pass_prompts_continue_a_non_empty_cache(product, oracle):
    """fp32 prompts of 129..192 tokens run every matrix in two passes of the stream kernels (plan_eval, round 6): the second pass's rows sit at
    positions past + ceil(n / 2).. of the RoPE table and the cache.  Chunks of 150 and 131 tokens behind 30 cached ones, then decode steps on
    the cache they wrote."""
    kw = dict(SHAPES["small"])
    kw["layers"] = 2
    hp = make_hparams(**kw, ctx=320)
    rng = np.random.default_rng(23)
    toks = [int(t) for t in rng.integers(0, kw["vocab"], 315)]
    chunks = [30, 150, 131, 1, 1]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 1234)
        c = m.NewContext(320, 16, False)
        out, past = [], 0
        for n in chunks:
            out.append(c.Eval(toks[past:past + n], past))
            past += n
        c.free()
        m.free()
        res[name] = out
    for k, (a, b) in enumerate(zip(res["hip"], res["orc"])):
        assert rel(a, b) <= TOL, k


@pytest.mark.parametrize("shape,prompt", [("tiny", [1, 5, 9, 200, 17, 3, 44, 100]), ("tiny", [7]), ("small", [1, 306, 1658, 278, 1593, 310, 834, 338])])
def test_greedy_decode_matches_oracle(product, oracle, shape, prompt):
    out = decode_both(product, oracle, shape, 64, prompt, 12)
    toks_h, lg_h = out["hip"]
    toks_o, lg_o = out["orc"]
    assert out["fused"] == 1, "the Eval graph was not recognised as a fused plan"
    assert rel(lg_h, lg_o) <= TOL
    assert toks_h == toks_o
    assert greedy_margin(lg_o) > 10 * TOL, "test seed has a near-tie; pick another"


@pytest.mark.parametrize("n_prompt", [2, 5, 8, 9, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128, 129, 130, 145, 161, 191, 192, 193])   # both sides of every launch-shape boundary, ragged last tiles (16 k - 1)
def test_prefill_mfma_path_matches_oracle(product, oracle, n_prompt):
    """One Eval of N tokens: 2..8 rows ride the decode weight stream (k_gemv_rows), 9..16 k_stream_mm2 (fp32 MFMA, RMSNorm folded), 17..48 and
    65..128 k_stream_dma (fp32 MFMA behind LDS-DMA loader waves), 49..64 k_stream_b9 (eight exact bf16 products per weight over activation
    planes, round 6), 129..192 k_stream_dma again in TWO passes of ceil(N / 2) rows per matrix (round 6) - RoPE / cache append / SiLU fused into
    the epilogues, ragged last column tile - and more rows the tile GEMMs + blocked attention; the next decode steps read the KV cache that
    prefill wrote."""
    rng = np.random.default_rng(n_prompt)
    prompt = [int(t) for t in rng.integers(0, SHAPES["small"]["vocab"], n_prompt)]
    out = decode_both(product, oracle, "small", 128 if n_prompt <= 120 else (192 if n_prompt <= 180 else 256), prompt, 4)
    toks_h, lg_h = out["hip"]
    toks_o, lg_o = out["orc"]
    assert out["fused"] == 1
    assert rel(lg_h, lg_o) <= TOL
    assert toks_h == toks_o


def test_long_prefill_dma_gemm_and_causal_skip_match_oracle(product, oracle):
    """Prompts long enough for every prefill GEMM to take the LDS-DMA kernel (contraction >= 512, incl. P.V over >= 512 keys) and
    for the attention GEMMs to skip fully masked tiles — in one Eval and continued from a non-empty cache (past > 0)."""
    kw = dict(SHAPES["small"])
    kw["layers"] = 2
    ctx = 640
    hp = make_hparams(**kw, ctx=ctx)
    rng = np.random.default_rng(7)
    prompt = [int(t) for t in rng.integers(0, kw["vocab"], 600)]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 1234)
        c = m.NewContext(ctx, 16, False)
        one = c.Eval(prompt, 0)                    # N = 600, past = 0
        nxt = c.Eval([5], 600)                     # decode step on the cache the prefill wrote
        c.free()
        c = m.NewContext(ctx, 16, False)
        c.Eval(prompt[:264], 0)
        two = c.Eval(prompt[264:], 264)            # N = 336, past = 264: P.V contracts over 608 (padded) keys
        c.free()
        m.free()
        res[name] = (one, nxt, two)
    for a, b in zip(res["hip"], res["orc"]):
        assert rel(a, b) <= TOL
    assert rel(res["hip"][0], res["hip"][2]) <= TOL   # chunked == single-shot


def test_prefill_attention_cut_by_key_range_matches_oracle(product, oracle):
    """The single-pass prefill attention cuts long query blocks into parts by key range when there are fewer blocks than workgroups
    or the causal triangle leaves them unbalanced (kernels_attn.h "Balance"; plan.hip flash_work_list): a long first Eval (every late
    block cut in two or more, the early ones whole), then chunks of a conversation behind a deep cache (one or three blocks, each
    cut into many parts), a ragged last block, and a decode step on the cache all of them wrote.  Each Eval against the restatement,
    and the chunked logits against a single Eval of the same 960 tokens."""
    kw = dict(SHAPES["small"])
    kw["layers"] = 2
    ctx = 1024
    hp = make_hparams(**kw, ctx=ctx)
    rng = np.random.default_rng(23)
    toks = [int(t) for t in rng.integers(0, kw["vocab"], 960)]
    chunks = [700, 64, 163, 33]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 1234)
        c = m.NewContext(ctx, 16, False)
        out, past = [], 0
        for n in chunks:
            out.append(c.Eval(toks[past:past + n], past))
            past += n
        out.append(c.Eval([7], past))
        c.free()
        if name == "hip":
            c = m.NewContext(ctx, 16, False)
            out.append(c.Eval(toks, 0))
            c.free()
        m.free()
        res[name] = out
    for a, b in zip(res["hip"], res["orc"]):
        assert rel(a, b) <= TOL
    assert rel(res["hip"][3], res["hip"][5]) <= TOL   # last chunk == single Eval of the 960 tokens


def test_generic_path_matches_fused_and_oracle(product, oracle):
    """Node-by-node execution of the very same graph (what an arbitrary ml graph gets) agrees with both."""
    hp = make_hparams(**SHAPES["tiny"], ctx=32)
    prompt = [1, 5, 9, 200, 17]
    m = product.NewSyntheticModel(hp, 99)
    mo = oracle.NewSyntheticModel(hp, 99)
    c = m.NewContext(32, 1)
    co = mo.NewContext(32, 1)
    ref = co.Eval(prompt, 0)
    os.environ["LLAMAGO_NO_FUSION"] = "1"
    try:
        got_generic = c.Eval(prompt, 0)
        assert product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h)) == 0
    finally:
        del os.environ["LLAMAGO_NO_FUSION"]
    c2 = m.NewContext(32, 1)
    got_fused = c2.Eval(prompt, 0)
    assert product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c2.h)) == 1
    assert rel(got_generic, ref) <= TOL
    assert rel(got_fused, ref) <= TOL
    # decode continuation on both caches
    r2 = co.Eval([42], 5)
    os.environ["LLAMAGO_NO_FUSION"] = "1"
    try:
        g2 = c.Eval([42], 5)
        assert product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h)) == 0   # the one-token step took the generic route too
    finally:
        del os.environ["LLAMAGO_NO_FUSION"]
    f2 = c2.Eval([42], 5)
    assert rel(g2, r2) <= TOL and rel(f2, r2) <= TOL
    for x in (c, c2, co):
        x.free()
    m.free()
    mo.free()


def test_weights_bit_identical_to_oracle(product, oracle):
    """The on-device synthetic generator and the oracle's CPU generator produce the same fp32 bits."""
    hp = make_hparams(**SHAPES["tiny"], ctx=16)
    m = product.NewSyntheticModel(hp, 4321)
    mo = oracle.NewSyntheticModel(hp, 4321)
    for name in ("tok_embeddings.weight", "norm.weight", "output.weight", "layers.1.attention.wq.weight", "layers.0.feed_forward.w2.weight", "layers.1.ffn_norm.weight"):
        a = product.read(None, m.tensor(name))
        b = oracle.read(None, mo.tensor(name))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    m.free()
    mo.free()


def test_resident_greedy_loop_equals_eval_loop(product):
    """Device-resident decode (argmax on the GPU, hipGraph replay, no host round trip) produces the same ids and
    final logits as the Eval-per-token loop of server.Do."""
    hp = make_hparams(**SHAPES["small"], ctx=64)
    m = product.NewSyntheticModel(hp, 7)
    c = m.NewContext(64, 1)
    prompt = [1, 306, 1658, 278]
    toks, lg = c.GreedyDecode(prompt, 10)
    c2 = m.NewContext(64, 1)
    c2.Eval(prompt, 0)
    first = int(np.argmax(c2.logits()))
    assert first == toks[0]
    out = (C.c_uint32 * 9)()
    last = np.empty(hp.vocabSize, np.float32)
    f = product.lib.llamago_DecodeGreedyResident
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    assert f(c2.h, first, len(prompt), 9, out, last.ctypes.data_as(C.POINTER(C.c_float))) == 0, product.last_error()
    assert list(out) == toks[1:]
    assert np.array_equal(last, lg[-1])
    c.free()
    c2.free()
    m.free()


def test_kept_decode_graph_gives_the_bits_of_a_fresh_build(product):
    """llama_Eval keeps the graph of a one-token Eval and moves it to the next position instead of building ~1700 tensors per token
    (host/llamago.cpp, eval_cache).  Same context, same positions, the kept graph on and off (llamago_KeepDecodeGraph): logits and the
    embedding row bit for bit - from the first position of the window to its last, across a prompt in between (the kept graph must
    survive Evals of other shapes), with the embedding output switched on half way (a different graph: the kept one is rebuilt)."""
    product.lib.llamago_KeepDecodeGraph.restype = None
    product.lib.llamago_KeepDecodeGraph.argtypes = [C.c_int]
    hp = make_hparams(**SHAPES["small"], ctx=40)
    m = product.NewSyntheticModel(hp, 7)
    runs = {}
    try:
        for keep in (1, 0):
            product.lib.llamago_KeepDecodeGraph(keep)
            c = m.NewContext(40, 1)
            out = []
            tok = 5
            for past in range(0, 12):                       # decode from an empty context
                lg = c.Eval([tok], past); out.append(lg.copy()); tok = int(np.argmax(lg))
            lg = c.Eval([3, 1658, 278, 9, 11], 12); out.append(lg.copy())   # a prompt in between
            c.EnableEmbedding()
            tok = int(np.argmax(lg))
            for past in range(17, 40):                      # ... and on to the last position of the window
                lg = c.Eval([tok], past); out.append(lg.copy()); out.append(c.Embedding().copy()); tok = int(np.argmax(lg))
            with pytest.raises(Exception):
                c.Eval([tok], 40)
            runs[keep] = out
            c.free()
    finally:
        product.lib.llamago_KeepDecodeGraph(1)
    m.free()
    assert len(runs[0]) == len(runs[1])
    for k, (a, b) in enumerate(zip(runs[1], runs[0])):
        assert np.array_equal(a, b), k


def test_ggjt_roundtrip_through_hbm(product, oracle, tmp_path):
    """Model written by the oracle as ggjt v1 (f32 and f16), loaded by the product loader straight into HBM,
    evaluates like the oracle's own load of the same file (llama.go:712-976)."""
    hp = make_hparams(**SHAPES["tiny"], ctx=32)
    mo = oracle.NewSyntheticModel(hp, 5)
    for ftype in (0, 1):
        path = str(tmp_path / f"tiny-{ftype}.bin")
        mo.Save(path, ftype)
        lo = oracle.LoadModel(path, 32)
        lp = product.LoadModel(path, 32)
        assert lp.hp.embdSize == hp.embdSize and lp.ffSize == mo.ffSize
        co, cp = lo.NewContext(32, 1), lp.NewContext(32, 1)
        a, b = cp.Eval([1, 2, 3], 0), co.Eval([1, 2, 3], 0)
        assert rel(a, b) <= TOL
        co.free(); cp.free(); lo.free(); lp.free()
    mo.free()


def test_product_loader_reads_the_reference_converter_files(product, oracle):
    """The ggjt files the REFERENCE's converter wrote (tests/golden/make_ggjt_from_reference.py: f32 one part, f16 two parts) through
    the product loader into HBM: weights bit-identical to the fixture state dict, greedy ids and logits equal to the checker's load
    of the same file, and to the independent numpy float64 forward."""
    import test_ggjt_reference_fixture as fxt
    from test_oracle import np_eval, np_weights
    models = fxt._check_loaded_model(product)       # hparams + every tensor, read back from HBM, == numpy rebuild of the state dict
    prompt = [1, 70, 261, 5, 280, 33, 9]
    for (mp, hp), fname in zip(models, fxt.FILES):
        mo = oracle.LoadModel(os.path.join(fxt.GOLDEN, fname), 32)
        cp, co = mp.NewContext(32, 1), mo.NewContext(32, 2, False)
        tp, lp = cp.GreedyDecode(prompt, 6)
        to, lo = co.GreedyDecode(prompt, 6)
        assert tp == to
        assert rel(lp, lo) <= TOL
        W = np_weights(oracle, mo)
        L, d, H = hp.layersCount, hp.embdSize, hp.headsCount
        kc, vc = np.zeros((L, 32, H, d // H)), np.zeros((L, 32, H, d // H))
        want = np_eval(W, hp, prompt, 0, kc, vc)
        assert np.abs(lp[0] - want).max() / np.abs(want).max() < 1e-5
        cp.free(); co.free(); mp.free(); mo.free()


def test_committed_golden_vectors_on_the_gpu(product):
    """tests/golden/tiny_eval.npz (committed KAT of the checker: ids + logits of 8 greedy steps) reproduced by the HIP path without the
    checker in the loop: a drifted checker and a drifted product cannot agree with a committed file by accident."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_eval.npz"))
    hp = make_hparams(**SHAPES["tiny"], ctx=int(g["ctx"]))
    m = product.NewSyntheticModel(hp, int(g["seed"]))
    w2 = product.read(None, m.tensor("layers.1.feed_forward.w2.weight")).reshape(-1)[:64]
    assert np.array_equal(w2, g["w2_head"])
    c = m.NewContext(int(g["ctx"]), 1)
    toks, lg = c.GreedyDecode([int(t) for t in g["prompt"]], len(g["tokens"]))
    assert toks == [int(t) for t in g["tokens"]]
    assert rel(lg, g["logits"]) <= TOL
    c.free()
    m.free()


def test_compute_timers_count_every_contract_call(product):
    """lh_ctx_time_computes / lh_ctx_compute_stats: one entry per lh_graph_compute, device time inside host time, sums zeroed by a re-arm."""
    hp = make_hparams(**SHAPES["small"], ctx=32)
    m = product.NewSyntheticModel(hp, 5)
    c = m.NewContext(32, 1)
    c.Eval([1, 2, 3], 0)                      # timers off: nothing counted
    assert c.ComputeStats()["calls"] == 0
    c.TimeComputes(True)
    c.Eval([1, 2, 3, 4], 0)
    for i in range(5):
        c.Eval([7 + i], 4 + i)
    st = c.ComputeStats()
    assert st["calls"] == 6
    assert 0 < st["device_us"] <= st["wall_us"] < 1e6
    c.TimeComputes(True)
    assert c.ComputeStats() == {"calls": 0, "wall_us": 0.0, "device_us": 0.0}
    c.TimeComputes(False)
    c.Eval([3], 9)
    assert c.ComputeStats()["calls"] == 0
    c.free(); m.free()


@pytest.mark.parametrize("n_prompt", [1, 3, 8, 20, 70, 130])
def test_embeddings_of_a_fused_eval_match_oracle(product, oracle, n_prompt):
    """lctx.Embedding (llama.go:381, 414-419): row N-1 of the final norm * weight rows.  The fused plan's lm_head launches never write those
    rows out; the Eval graph flags the node LH_T_OUTPUT and the plan materialises it - for every route an Eval takes (decode step, rows
    kernel, stream kernels, tile GEMM), prompt and the decode steps behind it."""
    hp = make_hparams(**SHAPES["small"], ctx=160)
    rng = np.random.default_rng(n_prompt)
    prompt = [int(t) for t in rng.integers(0, hp.vocabSize, n_prompt)]
    got = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 7)
        c = m.NewContext(160, 16, False)
        c.EnableEmbedding()
        lg = c.Eval(prompt, 0)
        e0 = c.Embedding()
        tok = int(np.argmax(lg))
        lg1 = c.Eval([tok], n_prompt)
        e1 = c.Embedding()
        if name == "hip":
            product.lib.llamago_LastGraphFused.restype = C.c_int
            product.lib.llamago_LastGraphFused.argtypes = [C.c_void_p]
            assert product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h)) == 1, "the flagged Eval graph must stay on the fused plan"
        got[name] = (e0, e1, lg, lg1)
        c.free()
        m.free()
    for k in range(4):
        assert rel(got["hip"][k], got["orc"][k]) <= TOL, k


def test_out_of_range_token_is_an_error_not_a_gpu_fault(product):
    """A token id >= vocab makes Go panic on the embedding slice (ml.go:1748); here it must come back as an error."""
    hp = make_hparams(**SHAPES["tiny"], ctx=8)
    m = product.NewSyntheticModel(hp, 1)
    c = m.NewContext(8, 1)
    with pytest.raises(Exception):
        c.Eval([1, hp.vocabSize + 5], 0)
    assert "GetRows" in product.last_error() or "outside" in product.last_error()
    c.Eval([1, 2], 0)  # the context is still usable
    c.free()
    m.free()


def test_context_overflow_is_an_error_not_a_crash(product):
    hp = make_hparams(**SHAPES["tiny"], ctx=8)
    m = product.NewSyntheticModel(hp, 1)
    c = m.NewContext(8, 1)
    c.Eval([1, 2, 3, 4, 5, 6, 7, 8], 0)
    with pytest.raises(Exception):
        c.Eval([9], 8)
    c.free()
    m.free()


@pytest.mark.parametrize("layers", [2])
def test_7b_shape_slice_matches_oracle(product, oracle, layers):
    """LLaMA-7B layer shape (d 4096, 32 heads, ff 11008, vocab 32000) truncated to a few layers so the oracle finishes
    in seconds: prefill of the 8-token benchmark prompt + 4 decode steps."""
    out = decode_both(product, oracle, "7B", 32, PROMPT, 5, layers=layers, threads=64)
    toks_h, lg_h = out["hip"]
    toks_o, lg_o = out["orc"]
    assert out["fused"] == 1
    assert rel(lg_h, lg_o) <= TOL
    assert toks_h == toks_o


@pytest.mark.parametrize("int8", [False, True])
def test_headline_workload_at_full_depth(product, int8):
    """BASELINE config 2 (and 4) ITSELF, not a slice: all 32 layers of LLaMA-7B, synthetic weights seed 1234, the fixed 8-token prompt,
    context 128, 100 greedy steps - through BOTH routes a caller has: the device-resident loop (lh_llama_decode_greedy) and one
    ml_GraphCompute per token (what server.Do's loop does, pkg/server/server.go:153-217).  The ids must equal the committed ones, which the
    checker decoded on its own (tests/golden/7b_seed1234[_int8]_ids.json: `oracle_ids_match`, written by tools/make_golden_ids.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = json.load(open(os.path.join(root, "tests", "golden", "7b_seed1234_int8_ids.json" if int8 else "7b_seed1234_ids.json")))
    assert gold["oracle_ids_match"] and gold["oracle_steps"] == len(gold["ids"]) == 100
    assert gold["min_top2_margin_rel"] > TOL, "the checker's own logits have a near-tie on the golden run"   # (fp32 1.3e-3, int8 1.5e-4; GPU vs checker 6e-6)
    hp = make_hparams(**SHAPES["7B"], ctx=128)
    m = product.NewSyntheticModel(hp, 1234)
    if int8:
        m.QuantizeQ8()
    c = m.NewContext(128, 1)
    first = int(np.argmax(c.Eval(PROMPT, 0)))
    toks, _ = decode_greedy_resident(c, first, len(PROMPT), 99)
    assert [first] + toks == gold["ids"], "device-resident loop"
    c.free()
    c = m.NewContext(128, 1)
    ids, tok = [], None
    for i in range(100):
        lg = c.Eval(PROMPT, 0) if i == 0 else c.Eval([tok], len(PROMPT) + i - 1)
        tok = int(np.argmax(lg))
        ids.append(tok)
    assert ids == gold["ids"], "one ml_GraphCompute per token"
    c.free()
    m.free()


@pytest.mark.parametrize("n_prompt", [3, 6, 8, 12, 24, 40, 49, 56, 64, 72, 90, 97, 112, 127, 128, 129, 160, 193])
def test_7b_shape_slice_short_prompts_match_oracle(product, oracle, n_prompt):
    """The 7B layer shape at the prompt lengths where the launch shape changes: 3 / 6 / 8 rows (the decode weight stream with four / eight
    activation rows), 12 rows (MFMA stream kernel, RMSNorm folded into the GEMMs), 24 rows (two column tiles, LDS-DMA loader waves; wo / w2 as
    K-split pairs + reduce pass that writes the next norm), 40 rows (three column tiles), 49 / 56 / 64 rows (four: k_stream_b9 over planes, wo / w2 as K-split fours), 72 / 90 rows (five / six),
    97 / 112 / 127 / 128 rows (eight column tiles, MFMA waves as 2 K-groups x 2 column halves), 129 / 160 rows (two passes of 65 + 64 / 80 + 80
    rows per matrix), 193 rows (the tile GEMM) - 2 layers, then 2 decode steps on the cache the prompt wrote."""
    rng = np.random.default_rng(100 + n_prompt)
    prompt = [int(t) for t in rng.integers(0, SHAPES["7B"]["vocab"], n_prompt)]
    out = decode_both(product, oracle, "7B", 64 if n_prompt <= 56 else (128 if n_prompt <= 120 else (192 if n_prompt <= 180 else 256)), prompt, 3, layers=2, threads=64)
    toks_h, lg_h = out["hip"]
    toks_o, lg_o = out["orc"]
    assert out["fused"] == 1
    assert rel(lg_h, lg_o) <= TOL
    assert greedy_margin(lg_o) > MARGIN, "the checker's own logits have a near-tie: pick another prompt seed (tools/check_test_margins.py)"
    assert toks_h == toks_o


@pytest.mark.parametrize("shape,layers,ctx", [("tiny", None, 32), ("small", None, 64), ("7B", 2, 32)])
def test_block_int8_weights_match_dequantised_oracle(product, oracle, shape, layers, ctx):
    """BASELINE config 4: block-int8 weight matrices (format ours: the reference has none).  The checker runs the fp32 path on
    the dequantised weights; the GPU streams int8 planes + scales and must agree (token ids exact, 1e-4 on logits)."""
    kw = dict(SHAPES[shape])
    if layers:
        kw["layers"] = layers
    hp = make_hparams(**kw, ctx=ctx)
    prompt = [1, 5, 9, 200, 17, 3, 44, 100] if shape != "7B" else PROMPT
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 321).QuantizeQ8()
        if name == "hip":
            wq_h = product.read(None, m.tensor("layers.1.attention.wq.weight"))
        else:
            wq_o = oracle.read(None, m.tensor("layers.1.attention.wq.weight"))
        c = m.NewContext(ctx, 64, False)
        res[name] = c.GreedyDecode(prompt, 6)
        c.free()
        m.free()
    assert np.array_equal(wq_h, wq_o), "GPU and CPU quantisers disagree"  # value equality: int8 0 has no sign, rint() may give -0.0
    (th, lh_), (to, lo) = res["hip"], res["orc"]
    assert rel(lh_, lo) <= TOL
    assert th == to


@pytest.mark.parametrize("shape,n_prompt", [("small", 3), ("small", 8), ("small", 16), ("small", 20), ("small", 32), ("small", 33), ("small", 45), ("small", 48), ("small", 88), ("small", 89), ("small", 100), ("small", 300), ("13B", 72),
                                            ("13B", 24), ("13B", 260), ("small", 129)])
def test_block_int8_prefill_gemm_matches_dequantised_oracle(product, oracle, shape, n_prompt):
    """Prompts of more than 128 tokens on a block-int8 model run a tile GEMM - k_gemm_q8b3 (int8 x three bf16 planes of the activations,
    three exact-product MFMAs per quant block) where its 128 x 256 tiles pay, else the dequantising k_gemm_q8 (int8 + scale -> fl32(d*q) ->
    LDS -> fp32 MFMA); 5..88 tokens k_stream_q8b (two 64-row passes from 65), from 89 one 128-row tile of k_gemm_q8b3; single rows the int8 GEMV stream.  Both must agree with the checker's
    dequantise-then-fp32 evaluation, and with each other on the cache they share."""
    kw = dict(SHAPES[shape])
    kw["layers"] = 2 if shape == "small" else 1     # 13B shape: 5120 = 32 x 160 columns -> the 128 x 160 tile variant
    hp = make_hparams(**kw, ctx=320)
    rng = np.random.default_rng(n_prompt)
    prompt = [int(t) for t in rng.integers(0, kw["vocab"], n_prompt)]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 321).QuantizeQ8()
        c = m.NewContext(320, 16, False)
        res[name] = c.GreedyDecode(prompt, 5)
        if name == "hip":  # the same prompt fed in chunks < 32 goes through the GEMV path only
            c2 = m.NewContext(320, 16, False)
            past = 0
            for i in range(0, n_prompt, 16):
                lg_chunked = c2.Eval(prompt[i:i + 16], past)
                past += len(prompt[i:i + 16])
            c2.free()
        c.free()
        m.free()
    (th, lh_), (to, lo) = res["hip"], res["orc"]
    assert rel(lh_, lo) <= TOL
    assert th == to
    assert rel(lg_chunked, lh_[0]) <= TOL


@pytest.mark.parametrize("shape", ["13B", "65B"])
def test_larger_shapes_slice_matches_oracle(product, oracle, shape):
    """13B (d 5120, ff 13824) and 65B (d 8192, ff 22016) layer shapes, 1 layer: exercises the KI = 2/4/6 column splits of the
    weight-streaming kernels and the small-N prefill with 4-row chunks."""
    out = decode_both(product, oracle, shape, 32, PROMPT, 3, layers=1, threads=64)
    toks_h, lg_h = out["hip"]
    toks_o, lg_o = out["orc"]
    assert out["fused"] == 1
    assert rel(lg_h, lg_o) <= TOL
    assert toks_h == toks_o


def test_long_context_split_attention_matches_oracle(product, oracle):
    """Plans with ctx > 256 decode with the split-T attention (chunks of 128 keys per workgroup + combine).  A 250-token prompt
    (MFMA prefill) followed by decode steps that cross the 256-key chunk boundary must match the oracle."""
    rng = np.random.default_rng(5)
    prompt = [int(t) for t in rng.integers(0, SHAPES["small"]["vocab"], 250)]
    out = decode_both(product, oracle, "small", 320, prompt, 12, threads=64)
    toks_h, lg_h = out["hip"]
    toks_o, lg_o = out["orc"]
    assert out["fused"] == 1
    assert rel(lg_h, lg_o) <= TOL
    assert toks_h == toks_o


@pytest.mark.parametrize("shape,layers", [("13B", 2), ("65B", 1)])
def test_config3_prefill_1024_tokens_matches_oracle(product, oracle, shape, layers):
    """BASELINE.json configs[2] at its stated size: 13B shape, 2-layer slice, ONE Eval of N = 1024 tokens at
    past = 0 (context 1025: room for the decode step behind it) — the run `bench.py`'s prefill_13b object times — plus a 65B-shape 1-layer slice.  Checker: the
    restatement with the reference's own AVX dot product over 16 host threads (the 1.1 TMAC scalar order would take minutes; both
    orders sit within 1e-5 of the float64 leg, tests/test_oracle.py).  Then one decode step on the cache the prefill wrote."""
    from llama_go_amd.mlapi import usable_threads
    kw = dict(SHAPES[shape])
    kw["layers"] = layers
    # N = 1024 exactly (the run the bench times: full 128-row tiles of k_gemm_b9 on the 13B shape) in a window of 1025, so that one decode step fits behind it
    hp = make_hparams(**kw, ctx=1025)
    toks = [int(t) for t in np.random.default_rng(0).integers(0, kw["vocab"], 1024)]
    res = {}
    for name, lib in (("hip", product), ("orc", oracle)):
        m = lib.NewSyntheticModel(hp, 1234)
        c = m.NewContext(1025, usable_threads(), True)
        a = c.Eval(toks, 0)
        b = c.Eval([int(np.argmax(a))], 1024)
        res[name] = (a, b)
        if name == "hip":
            product.lib.llamago_LastGraphFused.restype = C.c_int
            product.lib.llamago_LastGraphFused.argtypes = [C.c_void_p]
            assert product.lib.llamago_LastGraphFused(product.lib.llama_MLContext(c.h)) == 1
        c.free()
        m.free()
    for a, b in zip(res["hip"], res["orc"]):
        assert rel(a, b) <= TOL
        assert int(np.argmax(a)) == int(np.argmax(b))
