"""Long-lived contexts and batches held to fresh twins across re-captures (tests/session_ref.py: the harness and its three oracles; tests/session_cases.py:
the scripts and the trigger table they cover; tests/test_session_cpu.py: the same harness over a toy backend and its mutants).

Every other GPU test runs its call on a fresh object.  Each test here runs one script - a server's life in miniature: prompts that grow, detours at a
rewound position, samplers reconfigured, lookup runs among plain ones, feeds and forks among ticks - on ONE object, and holds every step to an eager twin
(every plan of which is made under LLAMAHIP_NO_GRAPH=1, and which is seen to launch where the other replays), to a fresh twin that runs the essential steps only, and to the route trace: the step behind a trigger must capture
again, the same step repeated must replay.  All comparisons are byte equalities of everything a step returns; a failure names script, step, oracle and the
first differing element.  Measured on an MI355X: every case takes 0.03 - 0.7 s (the 4100-id run is the longest); DESIGN.md lists them.

All four weight types run every script (f16 through NarrowF16, block-int4 through QuantizeQ4); the switch scripts run for f16 and block-int4, the tile script for f16,
the pair scripts for the three pairs of session_ref.PAIRS.  The long-lived object alone gets the lh_ctx switches a script sets, and in front of every step its
context's weight images are filled with 0xFF (llamago_PoisonWeightImages): see session_ref.py.  A step's `want` / `wantnot` patterns - the kernel family it is there
for - are asserted on its route trace here.
"""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import session_cases as sc  # noqa: E402
from session_ref import MODEL_SEED, EnvPatch, ProductBackend, run_script  # noqa: E402

pytestmark = pytest.mark.gpu

# the calls that run (part of) their work from a captured graph, and so may capture: the resident loops, the lookup runs, a tick; and a one-token Eval
CAN_CAPTURE = ("Decode", "SampleDecode", "DecodeLookup", "SampleDecodeLookup", "DecodeSampleLookup", "Tick")
_TRACES = {}   # (script, weights) -> the long-lived object's trace of every step, for test_no_captured_step_sizes_a_gemm_buffer


def _model_maker(product):
    """-> (get(shape, weights, seed), the dict of what it made): one synthetic model per (shape, weight type, seed); f16 through NarrowF16, block-int4 through QuantizeQ4."""
    from llama_go_amd.mlapi import SHAPES, make_hparams
    made = {}

    def get(shape, weights, seed=MODEL_SEED):
        if (shape, weights, seed) not in made:
            m = product.NewSyntheticModel(make_hparams(**{**SHAPES, **sc.SHAPES}[shape], ctx=512), seed)
            if weights == "q8":
                m.QuantizeQ8()
            elif weights == "f16":
                m.NarrowF16()
            elif weights == "q4":
                m.QuantizeQ4()
            made[(shape, weights, seed)] = m
        return made[(shape, weights, seed)]

    return get, made


@pytest.fixture(scope="module")
def models(product):
    """One synthetic model per (shape, weight type, seed) for the whole module; contexts, batches and pairs come and go on them."""
    get, made = _model_maker(product)
    yield get
    for m in made.values():
        m.free()


def _run(name, weights, models, monkeypatch):
    report, script = [], sc.SCRIPTS[name](weights)
    try:
        _TRACES[(name, weights)] = run_script(script, ProductBackend(models, monkeypatch), weights, report=report)
    finally:
        print("\n".join(report))   # (pytest shows it for a failing case: which triggers fired, which steps replayed, up to the step that did not hold)
    for i, (st, trace) in enumerate(zip(script.steps, _TRACES[(name, weights)])):   # the kernel family each step is there for
        for rx in st.want:
            assert any(re.search(rx, e) for e in trace), f"script {name} [{weights}] step {i} ({st.call}): no launch matches {rx} among {sorted(set(trace))}"
        for rx in st.wantnot:
            bad = [e for e in trace if re.search(rx, e)]
            assert not bad, f"script {name} [{weights}] step {i} ({st.call}): launches {bad[0]}, which matches {rx}"
    return _TRACES[(name, weights)]


@pytest.mark.parametrize("name,weights", sc.CASES)
def test_session(name, weights, models, monkeypatch):
    _run(name, weights, models, monkeypatch)


def test_no_captured_step_sizes_a_gemm_buffer(models, monkeypatch):
    """launch_gemm returns on the prepare-only flag BEFORE it reaches ensure_splitk, and k_gemm_q8b3 / k_gemm_b9 size the xs3 planes in front of theirs
    only by accident of order - against the rule on grow_floats (a buffer that can be sized inside a capture is sized in front of the prepare-only
    return).  The code shows why neither is a hipMalloc under capture:
      - the prepare-only pass exists in ONE place, ensure_decode_graph, around enqueue_decode: a decode step's matmuls are gemv<> -> launch_gemv /
        the block-int8 GEMV, never a tile GEMM.  So the flag is never set when launch_gemm runs;
      - every other capture (batch_tick_unchecked, spec_pass, batch_spec_pass) captures a plan_eval directly, but only behind an EAGER pass of the same
        row count on the same context (Batch::warm, Spec::warm bit R, BatchSpec::warm bit pods x R), and the context's split-K buffer and planes only
        grow: whatever such a pass needs was sized by its eager twin before the capture began;
      - and those passes have at most 64 rows (BATCH_ROWS_MAX; 8 for a solo lookup pass): they take the Rows / Planes routes or Prefill's stream kernels,
        which size split-K in front of their own prepare-only return; the tile GEMMs start at 193 rows (fp32) and 89 (block-int8).
    The scripts show it by route trace: no step of a call that can capture - whatever it is declared, behind any trigger, at any row count the scripts
    reach - records a k_gemm_* launch or a split-K reduce pass of one, while the detours that cross into the tile GEMM do record them (so the trace would have shown one)."""
    for name, weights in sc.CASES:
        traces = _TRACES.get((name, weights)) or _run(name, weights, models, monkeypatch)
        for i, (st, trace) in enumerate(zip(sc.SCRIPTS[name](weights).steps, traces)):
            call = st.call.rpartition(".")[2]   # (a pair's steps name their side)
            if call in CAN_CAPTURE or (call == "Eval" and len(st.args["tokens"]) == 1):   # whatever it is declared: an `eager` lookup run captures its second pass
                bad = [e for e in trace if re.match(r"k_gemm_|k_splitk_reduce|k_split3_rows", e)]
                assert not bad, f"script {name} [{weights}] step {i} ({st.call}) can capture and launches {bad[0]}"
    # (f16 runs the fp32 tile GEMM over its widened image, block-int4 k_gemm_q8b3 over its expanded one: the entries are the twins', with the widening / expanding passes in front)
    for weights, want in (("f32", r"^k_gemm_glds<.*>/s([2-9]|\d\d)$"), ("q8", r"^k_gemm_q8b3<4>/s\d+$"), ("f16", r"^k_gemm_glds<.*>/s([2-9]|\d\d)$"), ("q4", r"^k_gemm_q8b3<4>/s\d+$")):
        script = sc.SCRIPTS["solo.growing_prompts"](weights)
        i = max(k for k, st in enumerate(script.steps) if st.fires and st.fires[-1] in ("ensure_splitk", "ensure_xs3"))
        trace = _TRACES[("solo.growing_prompts", weights)][i]
        assert any(re.match(want, e) for e in trace), f"solo.growing_prompts [{weights}] step {i}: no tile GEMM among {sorted(set(trace))}"
        if weights in sc.LIKE_F32:
            assert "k_splitk_reduce" in trace
        else:
            assert "k_split3_rows" in trace
        if weights in ("f16", "q4"):
            assert ("k_widen_f16" if weights == "f16" else "k_expand_q4") in trace
    # the tile script's own statement: with lh_ctx_set_f16_tiles on, the 193-row prompt takes the half kernel (each such step's `want` is asserted where it runs)
    tiles = sc.SCRIPTS["solo.tiles_and_stream"]("f16")
    assert sum(1 for st in tiles.steps if any("k_gemm_b9_h" in rx for rx in st.want)) == 2


def test_longer_window_in_a_fresh_process(built):
    """Whether ensure_rope_table grows anything depends on the process: the table is per device and head size and only grows, and in a whole-suite run earlier
    tests have long made a longer one, so `solo.longer_window_appears` above then fires nothing (it still holds decode across another context's life).  Here
    the same script runs in a child process that has made no context before: the table starts at 256 positions (abi.hip: the minimum) and the window of 512
    MUST grow it under the live decode graphs."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and f"longer window: {len(sc.WEIGHTS)} cases hold" in r.stdout, r.stdout[-3000:]


if __name__ == "__main__":   # the child of test_longer_window_in_a_fresh_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from llama_go_amd.mlapi import load_product
    get, made = _model_maker(load_product())

    for w in sc.WEIGHTS:
        rep = []
        try:
            run_script(sc.SCRIPTS["solo.longer_window_appears"](w), ProductBackend(get, EnvPatch()), w, report=rep)
        finally:
            print("\n".join(rep))
    print(f"longer window: {len(sc.WEIGHTS)} cases hold")
