"""The fast walks' threshold criterion (traverse.hip walk<true>, bfs_walk; open_threshold.hpp)
bit for bit against the oracle, at every launch shape the one-GPU evaluation picks by size:
4 097 bodies (the first size past the breadth-first walk: 4 bodies per wave), ~20 000 (16 per
wave), ~70 000 (64 per wave), 2 000 (bfs_walk); massless cells; a theta whose square leaves the
threshold form's range (the IEEE walk); the counting walk; the device self-test."""
import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from conftest import bits_equal

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "vx", "vy", "m")


def _engine(arrs, theta):
    eng = bh_amd.Engine(bh_amd.default_params(theta=theta), device=0)
    eng.reset_bodies(*arrs)
    return eng


def _assert_state_equal(eng, ref):
    got, want = eng.get_bodies(), ref.get_bodies()
    assert len(got[0]) == len(want[0])
    for k, name in enumerate(FIELDS):
        bad = np.flatnonzero(got[k].view(np.int64) != want[k].view(np.int64))
        assert bad.size == 0, f"{name}: {bad.size} words differ, first at {bad[:5]}"


def _check(arrs, theta, steps=2):
    """One evaluation of the production walk, then `steps` steps (the pipelined step's kick-drift
    and kick-only walks), each against the oracle."""
    ref = oracle.Oracle(*arrs, theta=theta)
    rax, ray = ref.accelerations()
    eng = _engine(arrs, theta)
    ax, ay = eng.compute_accelerations()
    eng.close()
    bad = np.flatnonzero(ax.view(np.int64) != rax.view(np.int64))
    assert bad.size == 0, f"ax: {bad.size} words differ, first at {bad[:5]}"
    assert bits_equal(ay, ray)
    eng = _engine(arrs, theta)  # (a fresh start: the evaluation's build may have jittered bodies)
    ref = oracle.Oracle(*arrs, theta=theta)
    eng.step(steps)
    ref.step(steps)
    _assert_state_equal(eng, ref)
    eng.close()
    ref.close()


# (bodies of the two disks, bodies per wave of the launch)
SIZES = {4097: (3277, 820, 4), 20000: (16000, 4000, 16), 70000: (56000, 14000, 64)}


@pytest.mark.parametrize("n,theta", [(4097, 0.5), (4097, 0.3), (20000, 0.5), (20000, 0.3),
                                     (70000, 0.5), (70000, 0.3),
                                     (4097, 0.75), (4097, 1.0), (4097, 1.6),
                                     (20000, 0.75), (20000, 1.0), (20000, 1.6)])
def test_two_disks_cursor_walk(n, theta):
    n1, n2, bpw = SIZES[n]
    assert n1 + n2 == n
    plan = bh_amd.launch_plan(n, bh_amd.default_params(theta=theta))
    assert plan["bfs"] == 0 and plan["bpw"] == bpw, plan
    _check(scenes.two_disks(n1, n2), theta)


@pytest.mark.parametrize("theta", [0.5, 0.3, 1.0])
def test_two_disks_breadth_first_walk(theta):
    plan = bh_amd.launch_plan(2000, bh_amd.default_params(theta=theta))
    assert plan["bfs"] == 1, plan
    _check(scenes.two_disks(1000, 1000), theta)


@pytest.mark.parametrize("theta", [0.5, 1.0])
def test_massless_cells_take_the_leaf_threshold(theta):
    """Cells whose bodies all have negative mass are mass-0 records with the leaf flag
    (NODE_SKIP | NODE_LEAF): the threshold compare accepts them for every lane, their term is an
    exact +-0 and the cursor passes their subtree -- the bodies inside are never reached."""
    rng = np.random.default_rng(91)
    x, y, vx, vy, m = (a.copy() for a in scenes.uniform(30_000, 0.5, seed=90))
    for _ in range(25):
        cx, cy, half = rng.uniform(0, 2400), rng.uniform(0, 800), rng.uniform(2.0, 30.0)
        inside = (np.abs(x - cx) < half) & (np.abs(y - cy) < half)
        m[inside] = -rng.uniform(0.1, 0.9, inside.sum())
    _check((x, y, vx, vy, m), theta, steps=3)


@pytest.mark.parametrize("theta", [1e-200, 1e-100])
def test_theta_outside_the_threshold_range(theta):
    """theta = 1e-200: theta^2 underflows to zero, which the precondition refuses (and the engine
    evaluates as all pairs).  theta = 1e-100: theta^2 = 1e-200 < 2^-400 is refused too and the
    launch takes the IEEE walk, which opens every cell.  Both match the oracle."""
    _check(scenes.two_disks(200, 100), theta)


def test_counting_walk_visits_and_counters():
    arrs = scenes.two_disks(3277, 820)
    ref = oracle.Oracle(*arrs, theta=0.5)
    rax, ray, rvis = ref.accelerations(visits=True)
    ref.close()
    eng = _engine(arrs, 0.5)
    ax, ay, vis = eng.compute_accelerations(visits=True)
    c = eng.traversal_counters()
    eng.close()
    assert bits_equal(ax, rax) and bits_equal(ay, ray)
    assert np.array_equal(vis, rvis), "node-visit counts differ"
    assert c["lane_visits"] == int(rvis.sum())
    assert c["waves"] == (len(rvis) + 63) // 64
    assert c["wave_iters"] * 64 >= c["lane_visits"] > 0
    assert 0 < c["wave_blocks"] <= c["wave_iters"]


def test_selftest_covers_both_criterion_forms():
    """bh_selftest_fast_math also evaluates the product form and the threshold form of the
    criterion on generated operands (every depth, +-2 ulp around the threshold): 0 disagreements."""
    assert bh_amd.selftest_fast_math(1 << 24, seed=20261020) == 0
