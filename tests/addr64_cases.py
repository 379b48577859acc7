"""Cases that only tests/test_gpu_addr64.py's child processes run, on the library built with
BH_NODE_OFF32_LIMIT=0 (lib_addr64/): the scenes the 64-bit node-address walks need and no module
of the suite steps in just this way.  Collected only when named (the file name is no test
module's), they use the suite's own helpers and comparisons: the C oracle's state after the call
bit for bit, tests/walk_model.py's visit counts exactly, the groups checker exactly.
"""
import os

import numpy as np
import pytest

import bh_amd
import test_launch_plan as lp
import walk_model
from bh_amd import scenes
from conftest import bits_equal
from test_gpu_groups import CFG as GROUPS_CFG
from test_gpu_groups import check as check_groups
from test_gpu_launch_shapes import _advance, _evaluate, _ladder_scene
from test_gpu_neighbors import _dozen
from test_gpu_parity import FIELDS, _assert_acc_equal, _pair
from test_neighbors_ref import candidates
from test_step_log_ref import golden_start

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _variant_only():
    plan = bh_amd.launch_plan(2000)
    assert plan["node_addr64"] == 1 and plan["bfs"] == 0, \
        f"these cases are for the 64-bit node-address variant, not {bh_amd.LIB_PATH}"


def _golden_state(z, k):
    return tuple(z[f"k{k}_{f}"] for f in FIELDS)


def _assert_golden(eng, z, k):
    for name, got, want in zip(FIELDS, eng.get_bodies(), _golden_state(z, k)):
        assert bits_equal(got, want), f"{name} after {k} steps differs from the golden file"


# ---- a. the step on one GPU --------------------------------------------------------------------

def test_c1_baseline_ten_steps_in_one_call():
    """2000 bodies: the first walk is the cursor walk at one body per wave with the kick and the
    drift fused -- the stock library walks this size breadth first."""
    plan = lp.plan(2000)
    assert (plan["bfs"], plan["bpw"], plan["kick_bpw"]) == (0, 1, 1)
    eng, ref = _pair(scenes.config_scene("c1_baseline"), theta=0.5)
    try:
        _advance(eng, ref, (10,))
        _assert_golden(eng, np.load(os.path.join(GOLDEN, "c1_baseline_theta05.npz")), 10)
    finally:
        eng.close()
        ref.close()


def test_c1_baseline_ten_one_step_calls():
    eng, ref = _pair(scenes.config_scene("c1_baseline"), theta=0.5)
    try:
        _advance(eng, ref, (1,) * 10)
        _assert_golden(eng, np.load(os.path.join(GOLDEN, "c1_baseline_theta05.npz")), 10)
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("name,calls", [("merge_127", (4, 2)), ("jitter_306", (1, 2, 2)),
                                        ("outside_153", (2, 8))])
def test_golden_scene_steps(name, calls):
    """merge_127 stepped as test_gpu_radial_profile steps it (bodies are removed inside the first
    call); the jitter and the outside-the-root scenes up to a state their golden file holds."""
    arrs, cfg = golden_start(name + ".npz")
    eng, ref = _pair(arrs, **cfg)
    try:
        _advance(eng, ref, calls)
        if name == "merge_127":
            assert eng.num_bodies() < len(arrs[0])
        else:
            _assert_golden(eng, np.load(os.path.join(GOLDEN, name + ".npz")), sum(calls))
    finally:
        eng.close()
        ref.close()


def _wpb_switch():
    b = lp.field_boundaries("wpb", 2, 70_000)
    assert len(b) == 1
    return b[0]


@pytest.mark.parametrize("below", [1, 0])
def test_last_size_of_one_wave_per_workgroup_and_first_of_eight(below):
    """b - 1 and b where the plan takes the first walk from one wave per workgroup to eight, which
    is also where its waves become full (bodies_per_wave and waves_per_group, traverse.hip):
    test_ladder's scene and comparisons -- one evaluation, two steps in one call, one more."""
    b = _wpb_switch()
    n = b - below
    plan = lp.plan(n)
    assert (plan["bpw"], plan["wpb"]) == ((32, 1) if below else (64, 8)), plan
    assert (plan["kick_bpw"], plan["kick_wpb"]) == (plan["bpw"], plan["wpb"])
    eng, ref = _pair(_ladder_scene(n), theta=0.5)
    try:
        assert eng.num_bodies() == n
        _evaluate(eng, ref)
        _advance(eng, ref, (2, 1))
    finally:
        eng.close()
        ref.close()


# ---- b. bh_compute_accelerations and the counting walk -----------------------------------------

def test_two_disks_600_accelerations_and_visits():
    """The golden scene two_disks_600 at theta = 0.3: the production walk and the counting walk
    (64 bodies per wave, one wave per workgroup) against the oracle, the visit counts against the
    walk model as well, then the states the golden file holds after 1 and 20 steps."""
    z = np.load(os.path.join(GOLDEN, "two_disks_600_theta03.npz"))
    arrs, cfg = golden_start("two_disks_600_theta03.npz")
    assert cfg["theta"] == 0.3
    eng, ref = _pair(arrs, **cfg)
    try:
        vis = _assert_acc_equal(eng, ref)
        model = walk_model.walk_counts(arrs, theta=0.3)
        assert np.array_equal(vis, model.visits), "visit counts differ from the walk model"
        assert vis.min() > 0
        _advance(eng, ref, (1,))
        _assert_golden(eng, z, 1)
        _advance(eng, ref, (19,))
        _assert_golden(eng, z, 20)
    finally:
        eng.close()
        ref.close()


# ---- g. the group link walk over cells of mass 0 -----------------------------------------------

def test_groups_of_zero_and_negative_masses():
    """test_gpu_neighbors' dozen: two negative-mass bodies under an internal node of mass 0
    (NODE_SKIP), a body of mass 0, one outside the root cell."""
    arrs = _dozen()
    assert candidates(arrs, GROUPS_CFG)[0].tolist() == [0, 1, 2, 5, 8, 9, 11]
    for link in (0.0, 1.0, 20.0, 400.0, float("inf")):
        for min_members in (1, 2):
            check_groups(arrs, GROUPS_CFG, link, min_members)
