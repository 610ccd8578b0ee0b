"""not-gpu: the draft-model speculation rule (include/llamahip.h, lh_llama_decode_draft) as tests/draft_model_ref.py restates it, over toy models; the
mutants the harness must report; and the ABI of the new entry points (both headers declare them, both libraries export them, mlapi.py and the Go shim
bind them)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draft_model_ref as ref   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 97


def target(prefix):
    """A next-id function that depends on the whole prefix (position, last two tokens, a running sum)."""
    n = len(prefix)
    return (prefix[-1] * 31 + (prefix[-2] if n > 1 else 0) * 17 + sum(prefix) * 7 + n * 3 + 11) % V


def never(prefix):
    return (target(prefix) + 1) % V


def pattern(prefix):
    """Right except at every third position."""
    return target(prefix) if len(prefix) % 3 else (target(prefix) + 5) % V


def other(prefix):
    """A different function that agrees with the target now and then."""
    return target(prefix) if prefix[-1] % 2 else (prefix[-1] * 5 + len(prefix)) % V


DRAFTERS = {"equal": (target, dict(perfect=True)), "never": (never, dict(never=True)), "pattern": (pattern, {}), "other": (other, {})}
PROMPT = [5, 9, 2, 44, 7, 3, 90, 1]        # positions 0..7; the pending token is appended by the cases


@pytest.mark.parametrize("name", sorted(DRAFTERS))
@pytest.mark.parametrize("draft_len", range(1, 8))
def test_rule_equals_plain_greedy(name, draft_len):
    draft, kw = DRAFTERS[name]
    window = PROMPT + [13]
    past = len(PROMPT)
    for n_steps in (1, 2, draft_len, draft_len + 1, draft_len + 2, 23, 40):
        for ctx_t, ctx_d in ((64, 64), (64, past + n_steps), (past + n_steps, 64), (past + n_steps, past + n_steps), (past + n_steps + 1, past + n_steps + 3)):
            run = ref.check(target, draft, window, n_steps, draft_len, ctx_t, ctx_d, **kw)
            assert run["stats"]["rows"] == draft_len + 1
            if name == "equal":
                assert all(a == k for k, a in run["trace"]) and run["stats"]["passes"] == -(-n_steps // (draft_len + 1))
            if name == "never":
                assert run["stats"]["accepted"] == 0 and run["stats"]["passes"] == n_steps


def test_partial_acceptance_happens():
    tr = ref.check(target, pattern, PROMPT + [13], 40, 7, 64, 64)["trace"]
    assert any(0 < a < k for k, a in tr), tr
    tr = ref.check(target, other, PROMPT + [13], 40, 3, 64, 64)["trace"]
    assert sum(a for _, a in tr) > 0 and any(a < k for k, a in tr), tr


def test_target_shapes_that_lower_the_row_count():
    for rows_max, draft_len, want_rows in ((4, 7, 4), (1, 3, 1), (8, 7, 8), (2, 1, 2)):
        run = ref.check(target, pattern, PROMPT + [13], 20, draft_len, 64, 64, rows_max=rows_max)
        assert run["stats"]["rows"] == want_rows
        if want_rows == 1:      # plain greedy steps of the target, nothing drafted
            assert run["stats"] == dict(passes=20, rows=1, drafted=0, accepted=0, empty=20)


def test_a_run_past_either_window_is_refused():
    for ctx_t, ctx_d in ((64, 20), (20, 64)):
        with pytest.raises(ValueError):
            ref.decode_draft(target, target, PROMPT + [13], 13, 3, ctx_t, ctx_d)
        ref.check(target, target, PROMPT + [13], 12, 3, ctx_t, ctx_d)


def _reported(mutant, cases):
    hits = 0
    for draft, kw, n_steps, draft_len, ctx_t, ctx_d in cases:
        try:
            ref.check(target, draft, PROMPT + [13], n_steps, draft_len, ctx_t, ctx_d, mutant=mutant, **kw)
        except AssertionError:
            hits += 1
    return hits


def test_the_harness_reports_every_mutant():
    # no extra step: after a fully accepted pass the draft's cache lacks the row of the last accepted token
    assert _reported("no_extra_step", [(target, dict(perfect=True), 20, K, 64, 64) for K in range(1, 8)]) == 7
    # accept off by one: an id computed behind a wrong draft token is committed
    assert _reported("accept_off_by_one", [(never, {}, 20, K, 64, 64) for K in range(1, 8)]) == 7
    assert _reported("accept_off_by_one", [(pattern, {}, 40, 7, 64, 64)]) == 1
    # a limit that ignores the draft's window: steps (or filler rows) of the draft past the end of ITS cache
    past = len(PROMPT)
    assert _reported("limit_ignores_draft_window", [(target, {}, 20, K, 64, past + 10) for K in range(1, 8)]) == 7      # a run the rule refuses
    ragged = [K for K in range(1, 8) if 20 % (K + 1)]                                                                   # the last pass is clipped: filler rows
    assert _reported("limit_ignores_draft_window", [(target, {}, 20, K, 64, past + 20) for K in ragged]) == len(ragged) > 0
    # ... and the unmutated rule passes the very same cases
    for K in range(1, 8):
        ref.check(target, target, PROMPT + [13], 20, K, 64, 64, perfect=True)
        ref.check(target, never, PROMPT + [13], 20, K, 64, 64, never=True)
        ref.check(target, target, PROMPT + [13], 20, K, 64, past + 20)


# ---- ABI: the new entry points are declared, exported and bound --------------------------------------------------------------------------------
NEW_LH = ["lh_llama_decode_draft"]
NEW_GO = ["llamago_NewDraftPair", "llamago_FreeDraftPair", "llamago_DraftPairTarget", "llamago_DraftPairDraft", "llamago_DraftPairReplaceDraft",
          "llamago_DecodeDraft", "llamago_DecodeDraftContexts"]


def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b((?:lh|llamago)_[A-Za-z0-9_]+)\s*\(", src))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in ("T", "W")}


def test_headers_declare_and_libraries_export_the_draft_entry_points(built):
    import llama_go_amd as pkg
    assert set(NEW_LH) <= _decls("llamahip.h"), sorted(set(NEW_LH) - _decls("llamahip.h"))
    assert set(NEW_GO) <= _decls("llamago_ext.h"), sorted(set(NEW_GO) - _decls("llamago_ext.h"))
    assert set(NEW_LH) <= _exports(pkg.LIBLLAMAHIP)
    assert set(NEW_GO) <= _exports(pkg.LIBLLAMAGO)
    lib = C.CDLL(pkg.LIBLLAMAGO)
    assert all(hasattr(lib, n) for n in NEW_GO)
    py = open(os.path.join(ROOT, "llama.go_amd", "mlapi.py")).read()
    for n in NEW_GO:
        assert re.search(r"\bL\." + n + r"\b", py) or re.search(r"lib\." + n + r"\b", py), f"mlapi.py does not bind {n}"
    go = open(os.path.join(ROOT, "llama.go_amd", "go", "ml_hip_pods.go")).read()
    assert "C.lh_llama_decode_draft(" in go and "func (st *StageHIP) DecodeDraft(draft *StageHIP" in go


def test_the_header_states_the_rule_the_reference_restates():
    hdr = open(os.path.join(ROOT, "include", "llamahip.h")).read()
    for phrase in ("min(target window, draft window)", "The step j = k is there for the draft's cache row only", "trace[s] = (k_s << 8) | a_s",
                   "draft == target", "LH_EUNSUPPORTED"):
        assert phrase in hdr, phrase
