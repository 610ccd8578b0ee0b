"""The session harness proves it can fail (no GPU): tests/session_ref.py drives every script of tests/session_cases.py over the toy backend of
tests/session_toy.py.  The clean toy must pass all three oracles of every script; every mutant must be reported, by the oracle and at the step the
mutation first shows.  The trigger table is held to the scripts here too."""
import os
import re
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
    # the switches that choose a kernel.  Both values compute the same bytes by design, so a graph of the other value replayed behind a toggle changes nothing any twin
    # could see: the TRACE oracle is the one that must report a switch missing from the pass key, at the first run behind the toggle
    "switch_not_in_key": ("solo.switch_among_lookup_runs", 5, "oracle trace: declared eager", "f16"),
    # ... while a key that changes without the eager first pass shows in the bytes: the tick behind the toggle is captured with a kernel that never ran eagerly
    "warm_not_cleared": ("batch.switch_among_ticks", 5, "oracle eager twin: ids", "f16"),
    # the context-owned image: the first launch under the switch that reads its slot without filling it - a detour, which only the eager twin runs too, and the eager
    # twin is asked first.  test_the_fresh_twin_reports_an_unfilled_slot_too holds what the fresh twin says when it alone is asked, and
    # test_an_unfilled_image_slot_is_invisible_without_poison that only the poison makes the mutant visible
    "image_site_unfilled": ("solo.switch_among_lookup_runs", 7, "oracle eager twin: rows", "f16"),
    # a draft pair: the draft run behind the sampled detour samples (the fresh twin never ran the detour); the first resident run behind ReplaceDraft writes into a freed list
    "draft_leaves_smp": ("pair.draft_among_resident_runs", 15, "oracle fresh twin: ids", "f32"),
    "replace_frees_out": ("pair.replace_draft", 10, "oracle eager twin: ids", "f32"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_reported_at_its_step(mutant):
    name, step, oracle, w = (MUTANTS[mutant] + ("f32",))[:4]
    with pytest.raises(SessionMismatch) as e:
        run_script(sc.SCRIPTS[name](w), ToyBackend(mutant), w)
    msg = str(e.value)
    assert f"script {name} [{w}] step {step} " in msg and oracle in msg, msg


def test_an_unfilled_image_slot_is_invisible_without_poison():
    """The launch site that reads its image slot without filling it reads what the call before left there - the right matrix, with one model on the context: without
    the poison the mutant passes every oracle of every script of its weight type.  (With it, test_every_mutant_is_reported_at_its_step holds the report.)"""
    for name, w in sc.CASES:
        if w == "f16" and sc.SCRIPTS[name](w).kind != "pair":
            run_script(sc.SCRIPTS[name](w), ToyBackend("image_site_unfilled", poison=False), w)


def test_the_fresh_twin_reports_an_unfilled_slot_too():
    """The same mutant with the eager twin not asked: the fresh twin, which never runs the detours, reports it at the first ESSENTIAL step whose launch reads the
    unfilled slot - the 10-row prompt of the sampled lookup run under the switch - by its ids."""
    name, w = "solo.switch_among_lookup_runs", "f16"
    script = sc.SCRIPTS[name](w)
    step = next(i for i, st in enumerate(script.steps) if st.call == "SampleDecodeLookup")
    with pytest.raises(SessionMismatch) as e:
        run_script(script, ToyBackend("image_site_unfilled"), w, ask=("trace", "fresh", "repeat"))
    assert f"script {name} [{w}] step {step} " in str(e.value) and "oracle fresh twin: ids" in str(e.value), str(e.value)
    run_script(script, ToyBackend("image_site_unfilled", poison=False), w, ask=("trace", "fresh", "repeat"))


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
    for t, (where, what, expect, scripts, names) in sc.TRIGGERS.items():
        assert isinstance(names, tuple), t
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
    that is itself declared CAPTURE, or the EAGER first pass of a lookup run behind a change of the pass key, or the EAGER tick / run of the step that itself
    sets a stream switch, is the first of them.  For a lookup RUN this means that `recapture` is met by EAGER then REPLAY with no step declared CAPTURE: one call
    makes several passes - the first eager, the second captured, the rest replayed - and the trace of a call cannot tell them apart; run_script still demands
    launches of the EAGER run and none of the REPLAY run behind it."""
    for (name, w), script in _scripts().items():
        steps = script.steps
        for i, st in enumerate(steps):
            recaptured = False
            for entry in sorted(st.fires, key=lambda e: sc.TRIGGERS[e.split(">")[0]][2] != sc.RECAPTURE):
                t, _, family = entry.partition(">")
                seq = [s.trace for s in steps[i + 1:] if s.trace is not None and (not family or s.call == family)]
                if st.trace == CAPTURE or (st.trace == EAGER and not family and "Lookup" in st.call and "spec_key" in t) or \
                        (st.trace == EAGER and not family and t.endswith("_stream_switch") and st.env):   # (the step that sets the switch is the first run under it)
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
        assert script.doc and script.kind in ("solo", "batch", "pair") and script.ctx <= 384, name
        assert (script.kind == "pair") == ("." in script.steps[0].call), name   # (the steps of a pair, and only they, name their side)
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


# ---- the trigger table against the source ---------------------------------------------------------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.go_amd", "csrc")
SOURCES = ("plan.hip", "plan.h", "score.hip", "abi.hip", "comm.hip", "common.h", "graph_cache.h")


def _call_args(src, open_paren):
    depth, i = 0, open_paren
    while True:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        if depth == 0:
            return src[open_paren + 1:i]
        i += 1


def source_identifiers(sources):
    """What the table must answer for, read from the source text (comments stripped) of {file name: text}:
      - every identifier ending in _gen that is incremented (++x, x++, x += ...) or handed to grow( as the counter to bump (&..._gen)       -> "scratch_gen"
      - every field of every struct whose name ends in Key and that a CapturedGraph<...> is instantiated with                             -> "TickKey::shared", "Spec::Key::R"
        (a struct named just Key is qualified by the struct that encloses it)
      - the buffer of every grow( call that names a member (&p->emb; the helper's own forwarding call names a parameter and is skipped)     -> "p->emb" """
    found = set()
    for name, raw in sources.items():
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
        found |= set(re.findall(r"\+\+\s*(?:\w+(?:->|\.))*(\w+_gen)\b", src)) | set(re.findall(r"\b(\w+_gen)\s*(?:\+\+|\+=)", src))
        for m in re.finditer(r"\bgrow\(", src):
            args = [a.strip() for a in _call_args(src, m.end() - 1).split(",")]
            found |= {a.rsplit(">", 1)[-1].rsplit(".", 1)[-1] for a in args if re.fullmatch(r"&[\w>.-]+_gen", a)}
            found |= {a[1:] for a in [x for x in args[:2] if re.fullmatch(r"&\w+->\w+", x)][:1]}   # (the buffer is the first &owner->member: behind ctx, or in front in comm.hip's grow)
        graphs = set(re.findall(r"CapturedGraph<\s*([\w:]+)\s*>", src))
        for m in re.finditer(r"\bstruct\s+(\w*Key)\s*\{(.*?)\};", src, flags=re.S):
            key = m.group(1)
            if key == "Key":   # Spec::Key, BatchSpec::Key: the enclosing struct is the last one opened in front of it
                key = [o for o in re.findall(r"\bstruct\s+(\w+)\s*\{", src[:m.start()]) if o != "Key"][-1] + "::Key"
            assert key.split("::")[-1] in {g.split("::")[-1] for g in graphs} or key == "DecodeKey", f"{name}: struct {key} is no key of a CapturedGraph"
            for decl in m.group(2).split(";"):
                names = [d.split()[-1].lstrip("*") for d in decl.split(",") if d.strip()]
                found |= {f"{key}::{n}" for n in names}
    return found


def _read_sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in SOURCES}


def test_the_table_names_what_the_source_has():
    """Every generation counter, key field and grown buffer of the source is named by some row of the table, and no row names one the source does not have: the table
    is held to the source, not only to the scripts.  (With the rows of the two stream switches taken out this fails for f16_stream_gen, q4_stream_gen and the three
    f16_stream key fields - the state six merged changes had added without a row.)"""
    found = source_identifiers(_read_sources())
    assert {"scratch_gen", "out_gen", "DecodeKey::out_gen", "TickKey::x_in", "Spec::Key::lp", "BatchSpec::Key::ring_cap", "ctx->splitk", "cm->send_host"} <= found, sorted(found)
    named = {n: t for t, row in sc.TRIGGERS.items() for n in row[4]}
    missing = sorted(found - set(named))
    assert not missing, f"no row of session_cases.TRIGGERS answers for {missing}"
    stale = sorted(f"{n} (row {t})" for n, t in named.items() if n not in found)
    assert not stale, f"session_cases.TRIGGERS names what the source no longer has: {stale}"


def test_the_collector_sees_a_new_counter_a_new_key_field_and_a_new_buffer():
    """The collector on a source that gained one of each: all three are found (so the test above would fail until a row names them)."""
    src = _read_sources()
    before = source_identifiers(src)
    src["abi.hip"] += "\nint lh_ctx_set_new(lh_ctx* ctx) { ++ctx->new_switch_gen; return grow(ctx, &ctx->new_buf, &ctx->new_cap, 4, 4, 0, &ctx->new_buf_gen); }\n"
    src["plan.hip"], n = re.subn(r"(struct\s+TickKey\s*\{[^}]*?\buint64_t\s+f16_stream)\s*;", r"\1, new_field;", src["plan.hip"], count=1)
    assert n == 1, "plan.hip: no `uint64_t f16_stream;` in struct TickKey to extend"
    after = source_identifiers(src)
    assert after - before == {"new_switch_gen", "new_buf_gen", "ctx->new_buf", "TickKey::new_field"}, sorted(after - before)


# ---- the poison export: header, libraries, Python binding and Go shim agree (tests/test_abi.py holds headers and exports to each other in general) ---------------
def test_the_poison_export_is_declared_exported_and_bound(built):
    import ctypes as C
    import llama_go_amd as pkg
    from llama_go_amd import mlapi
    root = os.path.dirname(CSRC.rstrip("/")).rsplit("llama.go_amd", 1)[0]
    hip_hdr, ext_hdr = (open(os.path.join(root, "include", h)).read() for h in ("llamahip.h", "llamago_ext.h"))
    assert "int lh_ctx_poison_weight_images(lh_ctx* ctx, uint64_t* bytes);" in hip_hdr
    product_part = ext_hdr.split("[product] device plumbing", 1)[1]
    for name in ("llamago_PoisonWeightImages", "llamago_BatchPoisonWeightImages"):
        assert re.search(r"\bint64_t " + name + r"\(", product_part), name
    hip = C.CDLL(pkg.LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    hip.lh_ctx_poison_weight_images.restype, hip.lh_ctx_poison_weight_images.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64(7)
    assert hip.lh_ctx_poison_weight_images(None, C.byref(n)) == -1 and n.value == 7       # LH_EINVAL, nothing written
    go = C.CDLL(pkg.LIBLLAMAGO)
    for name in ("llamago_PoisonWeightImages", "llamago_BatchPoisonWeightImages"):
        f = getattr(go, name)
        f.restype, f.argtypes = C.c_int64, [C.c_void_p]
        assert f(None) == -1
    assert hasattr(mlapi.Context, "PoisonWeightImages") and hasattr(mlapi.Batch, "PoisonWeightImages")
    go_src = open(os.path.join(root, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    go_code = re.sub(r"//[^\n]*", "", go_src)
    assert re.search(r"func \(ctx \*Context\) PoisonWeightImagesHIP\(\) uint64 \{[^}]*C\.lh_ctx_poison_weight_images\(ctx\.hip\.ctx, &\w+\)", go_code)      # the context form ...
    assert re.search(r"func \(bt \*BatchHIP\) PoisonWeightImages\(\) uint64 \{\s*return bt\.ctx\.PoisonWeightImagesHIP\(\)\s*\}", go_code)                 # ... and the batch form over it
