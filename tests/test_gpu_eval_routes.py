"""The launch sequence of every Eval route, pinned to the one recorded before plan_eval (llama.go_amd/csrc/plan.hip) became a switch over eval_route
with one function per route: tests/eval_route_cases.py lists the calls - solo Evals on both sides of every route boundary, batch ticks, a verify pass,
first-only and last-only pipeline stages - tests/golden/eval_route_traces.json holds, per call, the matmul and attention instantiations mlapi.route_trace
saw, in order, as recorded on an MI355X at that earlier commit.  The route trace names the MFMA, split-K and attention launches with their template
arguments; the GEMV launches of the Step, Rows and Skinny routes are not in it, so those routes show as their attention entries alone.

The routes are functions of the device's CU count (tiles per workgroup): on a device with another count the test fails and says so."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_route_cases as ERC   # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_route_traces.json")) as _f:
    GOLD = json.load(_f)


def test_golden_lists_every_case():
    """The golden and the case list name the same models and calls; no call was recorded as an empty trace."""
    assert sorted(GOLD["traces"]) == sorted(ERC.model_key(s, w) for s, w in ERC.MODELS)
    for shape, wtype in ERC.MODELS:
        want = GOLD["traces"][ERC.model_key(shape, wtype)]
        assert sorted(want) == sorted(ERC.case_ids(shape, wtype)), (shape, wtype)
        assert all(want[cid] for cid in want), (shape, wtype, [cid for cid in want if not want[cid]])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,wtype", ERC.MODELS, ids=[ERC.model_key(s, w).replace("/", "-") for s, w in ERC.MODELS])
def test_eval_routes_launch_what_the_recorded_commit_launched(product, shape, wtype):
    cus = ERC.device_cus()
    assert cus == GOLD["num_cu"], f"the route traces were recorded on a device with {GOLD['num_cu']} CUs; this one has {cus}, and the routes depend on the count"
    got = ERC.run_model(product, shape, wtype)
    want = GOLD["traces"][ERC.model_key(shape, wtype)]
    assert sorted(got) == sorted(want)
    for cid in ERC.case_ids(shape, wtype):
        assert " ".join(got[cid]) == want[cid], f"{shape}/{wtype} {cid}: launched {' '.join(got[cid])}; recorded {want[cid]}"
