"""The prep kernel's regrouped phases on the host emulation (no GPU): the assembly's serial chain as phases of the first wavefront, x_k
folded into the state difference, q and the cold flag handed from the assembly to the scaling part in thread registers, the cone block in
LDS outside the union.  None of it may move a bit, and none of it may depend on the order in which the threads of a phase run or on what
a fresh workgroup finds in its registers and LDS.

Horizons 2 and 3 are there because the set-up scratch in xk / sdiff overlaps the arrays it feeds and the H - 1 loops are shortest; 10, 12,
16, 20 are the shipped configurations (12 and 10 differ in where q lives, 16 / 20 in the tiles per thread).  Five robots per horizon
(tools/mint_prep_fixtures.cases): the robot types and gaits mixed, a planning step with all four feet in swing, a NaN input in the second
call (NON_CVX, so the third call restarts cold).  The fixture was minted from the parent commit's emulation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mint_prep_fixtures as mint  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "prep_phases_emu_parent.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(FIXTURE))


@pytest.fixture(scope="module", params=mint.HORIZONS)
def runs(request):
    h = request.param
    return h, {mode: mint.run_emu(ROOT, h, reverse=(mode == "reverse"), poison=(mode == "poison")) for mode in ("forward", "reverse", "poison")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_cases_cover_what_they_claim(runs):
    h, res = runs
    cs = mint.cases(h, 5)
    from rl_mpc_locomotion_amd import layout as L
    assert len({int(g) for g in cs[0][0].gait_id}) > 1 and len({int(r) for r in cs[0][0].robot_type}) > 1
    assert all((rec[1, L.IN_CONTACT + 4 * (1 % h):L.IN_CONTACT + 4 * (1 % h) + 4] == 0).all() for _, rec in cs)
    assert np.isnan(cs[1][1][4]).any() and not np.isnan(cs[0][1]).any() and not np.isnan(cs[2][1]).any()
    info = [res["forward"][f"h{h}_c{c}_info"] for c in range(mint.CALLS)]
    assert (info[0][:, 5] == 1).all()                                  # the cold call
    assert info[1][4, 1] == -7 and (info[1][:4, 5] == 0).all()         # NON_CVX beside four warm solves ...
    assert info[2][4, 5] == 1 and (info[2][:4, 5] == 0).all()          # ... and its cold restart


def test_thread_order_and_poison_do_not_matter(runs):
    h, res = runs
    for key, v in res["forward"].items():
        assert same_bits(v, res["reverse"][key]), f"{key}: reversed thread order differs"
        assert same_bits(v, res["poison"][key]), f"{key}: poisoned registers / LDS differ"


def test_equals_the_parent(runs, golden):
    h, res = runs
    keys = [k for k in golden if k.startswith(f"h{h}_")]
    assert len(keys) == 3 * mint.CALLS
    for key in keys:
        assert same_bits(res["forward"][key], golden[key]), f"{key} differs from the parent commit's emulation"
