"""The session harness proves it can fail (no GPU): tests/session_ref.py drives every script of tests/session_cases.py over the toy backend of
tests/session_toy.py.  The clean toy must pass all three oracles of every script; every mutant must be reported, by the oracle and at the step the
mutation first shows.  The trigger table is held to the scripts here too."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import session_cases as sc  # noqa: E402
from session_ref import CAPTURE, DETOUR, EAGER, REPLAY, SessionMismatch, first_difference, run_script, swap_positions, toks  # noqa: E402
from session_toy import ToyBackend  # noqa: E402


@pytest.mark.parametrize("name,weights", sc.CASES)
def test_clean_toy_passes_every_script(name, weights):
    report = []
    run_script(sc.SCRIPTS[name](weights), ToyBackend(), weights, report=report)
    assert len(report) == len(sc.SCRIPTS[name](weights).steps)


# mutant -> (script, step index, oracle) of the report it must produce
MUTANTS = {
    "growth_keeps_graph": ("solo.growing_prompts", 4, "oracle trace: declared capture"),
    "partial_invalidation": ("solo.more_than_4096_ids", 4, "oracle eager twin: ids"),
    "variant_kept": ("solo.sampler_reconfiguration", 2, "oracle trace: declared capture"),
    "ring_not_reinit": ("batch.sampler_on_off_on", 16, "oracle fresh twin: rings"),
    "detour_leaves_row": ("solo.resident_around_detours", 7, "oracle fresh twin: ids"),
    "draw_not_restored": ("solo.sampler_reconfiguration", 1, "oracle repeat of step 0: ids"),
    # not a product mutant: the harness's own footing.  A twin that captures graphs like the long-lived object repeats a stale graph byte for byte, so the
    # harness must notice that its "eager" twin is not eager (a solo context makes its plans lazily, after an environment window around its creation closed)
    "twin_not_eager": ("solo.growing_prompts", 2, "oracle eager twin: the twin itself recorded no launch"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_reported_at_its_step(mutant):
    name, step, oracle = MUTANTS[mutant]
    with pytest.raises(SessionMismatch) as e:
        run_script(sc.SCRIPTS[name]("f32"), ToyBackend(mutant), "f32")
    msg = str(e.value)
    assert f"script {name} [f32] step {step} " in msg and oracle in msg, msg


def test_a_stale_graph_is_seen_by_the_eager_twin_where_the_trace_is_not_asked():
    """With the trace expectations taken away the growth mutant must still be reported: by the eager twin, at the first step that replays the stale graph,
    naming the first differing element."""
    import dataclasses
    script = sc.SCRIPTS["solo.growing_prompts"]("f32")
    blind = dataclasses.replace(script, steps=tuple(dataclasses.replace(s, trace=None) for s in script.steps))
    with pytest.raises(SessionMismatch) as e:
        run_script(blind, ToyBackend("growth_keeps_graph"), "f32")
    assert "step 4 " in str(e.value) and "oracle eager twin: logits[0]" in str(e.value), str(e.value)


def test_mutants_leave_the_other_scripts_alone():
    """A mutant is reported by the scripts that fire its trigger, not by all of them: the reports are specific."""
    run_script(sc.SCRIPTS["solo.longer_window_appears"]("f32"), ToyBackend("variant_kept"), "f32")
    run_script(sc.SCRIPTS["batch.batches_come_and_go"]("f32"), ToyBackend("ring_not_reinit"), "f32")


# ---- the trigger table ------------------------------------------------------------------------------------------------------------------------------------
def _scripts():
    return {(name, w): sc.SCRIPTS[name](w) for name, w in sc.CASES}


def test_every_trigger_is_covered_by_a_script_or_says_why_not():
    fired = {}
    for (name, w), script in _scripts().items():
        for st in script.steps:
            for t in (e.split(">")[0] for e in st.fires):
                assert t in sc.TRIGGERS, f"{name}: step fires {t}, which the trigger table does not list"
                fired.setdefault(t, set()).add(name)
    for t, (where, what, expect, scripts) in sc.TRIGGERS.items():
        assert where and what and expect in (sc.RECAPTURE, sc.KEEP), t
        if isinstance(scripts, str):
            assert scripts.startswith("not covered: ") and t not in fired, (t, scripts)
            continue
        assert scripts, f"trigger {t} names no script"
        for name in scripts:
            assert name in sc.SCRIPTS and name in fired.get(t, ()), f"trigger {t}: script {name} has no step that fires it"
        assert fired[t] == set(scripts), f"trigger {t}: fired by {sorted(fired[t])}, the table says {sorted(scripts)}"
    assert sc.TRIGGERS["pipeline_rows_cap"][3] == "not covered: needs ranks"


def test_every_firing_step_is_followed_by_its_trace_expectations():
    """Behind a step that fires a `recapture` trigger the next steps with a trace expectation (of the call a "name>Call" entry names) are declared CAPTURE
    (or EAGER: a first pass at a new row count) and then REPLAY; behind a step that fires only `keep` triggers the next one is declared REPLAY.  A step
    that is itself declared CAPTURE, or the EAGER first pass of a lookup run behind a change of the pass key, is the first of them."""
    for (name, w), script in _scripts().items():
        steps = script.steps
        for i, st in enumerate(steps):
            recaptured = False
            for entry in sorted(st.fires, key=lambda e: sc.TRIGGERS[e.split(">")[0]][2] != sc.RECAPTURE):
                t, _, family = entry.partition(">")
                seq = [s.trace for s in steps[i + 1:] if s.trace is not None and (not family or s.call == family)]
                if st.trace == CAPTURE or (st.trace == EAGER and not family and "Lookup" in st.call and "spec_key" in t):
                    seq = [st.trace] + seq
                where = f"{name}[{w}] step {i} ({st.call}) fires {entry}"
                if sc.TRIGGERS[t][2] == sc.RECAPTURE:
                    recaptured = True
                    k = 0
                    while k < len(seq) and seq[k] in (CAPTURE, EAGER):
                        k += 1
                    assert k >= 1 and seq[k:k + 1] == [REPLAY], f"{where}: followed by {seq[:k + 1]}, not by capture then replay"
                elif not recaptured:
                    assert seq[:1] == [REPLAY], f"{where}: followed by {seq[:1]}, not by a replay"


def test_scripts_are_well_formed():
    for (name, w), script in _scripts().items():
        assert script.doc and script.kind in ("solo", "batch") and script.ctx <= 384, name
        assert any(s.role == DETOUR for s in script.steps) or script.kind == "batch" or "sampler" in name or "4096" in name, f"{name} has no detour"
        assert any(s.trace == REPLAY for s in script.steps) and any(s.trace == CAPTURE for s in script.steps), f"{name} never replays"
        for i, s in enumerate(script.steps):
            assert s.equals is None or s.equals < i


def test_helpers():
    assert toks(5, 1, 512) == toks(5, 1, 512) and all(1 <= t < 512 for t in toks(200, 3, 512)) and toks(5, 1, 512) != toks(5, 2, 512)
    assert swap_positions(60, 3, 64, 8) == 63 and swap_positions(63, 2, 64, 8) == 8 + 28 + 1
    import numpy as np
    a = {"x": np.arange(6, dtype=np.float32).reshape(2, 3)}
    b = {"x": a["x"].copy()}
    assert first_difference(a, b) is None
    b["x"][1, 2] = np.nan
    assert first_difference(a, b).startswith("x[1, 2]: ")
    assert first_difference({"x": np.float32([np.nan])}, {"x": np.float32([np.nan])}) is None          # bytes, not values
    assert "differ" in first_difference(a, {"y": a["x"]})
