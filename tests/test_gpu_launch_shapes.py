"""GPU: every size-dispatched path of the one-GPU step at its boundaries, bit for bit against
the CPU oracle.

The step picks its kernels and launch shapes from the list size N (the one-workgroup build
front, the cell table's depth, buckets, chunks, span groups, the base scan, the breadth-first
first walk, bodies per wave, waves per workgroup, the XCD remap's tail).  The sizes tested here
are where bh_launch_plan changes, found by tests/test_launch_plan.py -- none is written down.
The breadth-first walk's three give-ups to the cursor walk are forced by scenes whose property
tests/walk_model.py shows on the reference's tree alone (tests/test_launch_plan.py).
"""
import functools

import numpy as np
import pytest

import bh_amd
import oracle
import test_launch_plan as lp
from bh_amd import scenes
from conftest import bits_equal
from test_gpu_parity import (_assert_arrays_equal, _assert_state_equal, _async_call, _pair,
                             _production_walk)

pytestmark = pytest.mark.gpu


def _assert_finite(what, *arrays):
    for a in arrays:
        assert np.all(np.isfinite(a)), f"the oracle's {what} is not finite"


def _evaluate(eng, ref, every=None):
    """test_gpu_parity's _assert_acc_equal -- production walk, counting walk, visit counts and
    the state after the build's jitter against the oracle -- with the oracle's results asserted
    finite first.  every: the oracle walks these bodies only (_assert_sampled_evaluation)."""
    rax, ray, rvis = ref.accelerations(subset=every, visits=True)
    _assert_finite("accelerations", rax, ray)
    _assert_finite("state after the build", *ref.get_bodies())
    pick = slice(None) if every is None else every
    fx, fy = _production_walk(eng)
    ax, ay, vis = eng.compute_accelerations(visits=True)
    for got, want, what in ((fx, rax, "production walk ax"), (fy, ray, "production walk ay"),
                            (ax, rax, "counting walk ax"), (ay, ray, "counting walk ay")):
        bad = np.flatnonzero(got[pick].view(np.int64) != want.view(np.int64))
        assert bad.size == 0, f"{what}: {bad.size} bodies differ, first at {bad[:5]}"
    assert np.array_equal(vis[pick], rvis), "node-visit counts differ"
    _assert_state_equal(eng, ref)


def _advance(eng, ref, calls):
    for k in calls:
        eng.step(k)
        ref.step(k)
        _assert_finite("state", *ref.get_bodies())
        _assert_state_equal(eng, ref)


# ---- a. the ladder ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ladder_bodies():
    """Two colliding disks, the two heavy centres first and the rest shuffled, so that any
    prefix holds both disks and the merge rule has work."""
    arrs = scenes.two_disks(35_000, 35_000)
    heavy = np.flatnonzero(arrs[4] > 4000.0)
    rest = np.setdiff1d(np.arange(len(arrs[0])), heavy)
    order = np.concatenate([heavy, np.random.default_rng(2024).permutation(rest)])
    return tuple(a[order] for a in arrs)


OUTSIDE = (np.array([-3.0, 2402.5, 1200.0]), np.array([400.0, 400.0, -802.5]),
           np.array([1.0, -2.0, 0.0]), np.array([0.0, 1.0, 3.0]), np.array([3.0, 2.0, 1.5]))


def _ladder_scene(n, offset=0):
    """n bodies: a prefix of the ladder's disks (from `offset`) and, from 5 bodies up, three
    bodies outside the root cell at the end of the list (never inserted, BHA:126: the tail of the
    sorted order and of the last wave)."""
    out = 3 if n >= 5 else 0
    base = _ladder_bodies()
    return tuple(np.concatenate([b[offset:offset + n - out], o[:out]])
                 for b, o in zip(base, OUTSIDE))


@pytest.mark.parametrize("n", lp.ladder_sizes())
def test_ladder(n):
    """b - 1 and b for every size b at which the plan switches a kernel or a wave shape, and
    2^k + 1: one evaluation, two steps in one call, one step more; merging on."""
    eng, ref = _pair(_ladder_scene(n), theta=0.5)
    try:
        assert eng.num_bodies() == n
        _evaluate(eng, ref)
        _advance(eng, ref, (2, 1))
    finally:
        eng.close()
        ref.close()


# ---- b. the high switches --------------------------------------------------------------------

def _high(field):
    b = lp.field_boundaries(field, 70_000, 5_000_000)
    assert b, f"{field} has no switch below 5e6 bodies"
    return b[0]


@pytest.mark.parametrize("field", ["wpb", "span_groups"])
@pytest.mark.parametrize("below", [1, 0])
def test_high_switch_every_body(field, below):
    """Waves per workgroup 8 -> 4 and span groups 1 -> 2: b - 1 and b, every body of a uniform
    scene against the oracle."""
    b = _high(field)
    assert lp.plan(b - 1)[field] != lp.plan(b)[field]
    n = b - below
    eng, ref = _pair(scenes.uniform(n, 1.0, seed=21), theta=0.5)
    try:
        _evaluate(eng, ref)
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("below", [1, 0])
def test_high_switch_own_scan(below):
    """The build's own scan of the node counts against the library's: b - 1 and b, sampled
    (_assert_sampled_evaluation's comparison, the oracle's results finite first)."""
    b = _high("own_scan")
    assert lp.plan(b - 1)["own_scan"] == 1 and lp.plan(b)["own_scan"] == 0
    n = b - below
    eng, ref = _pair(scenes.uniform(n, 1.0, seed=22), theta=0.5)
    try:
        _evaluate(eng, ref, every=np.arange(0, n, 1021, dtype=np.int64))
    finally:
        eng.close()
        ref.close()


# ---- c. the breadth-first walk's give-ups ------------------------------------------------------

@pytest.mark.parametrize("name", list(lp.GIVE_UP_SCENES))
def test_bfs_give_ups(name):
    """Scenes in which no body, every body or a part of the bodies of one launch leaves the
    breadth-first walk -- too many accepted nodes, too many opened cells on a level, a tree
    beyond the bitmap: the plain evaluation, three steps in one call (the drifting first walk,
    then the cursor kick-only walk), and three one-step calls with the mirror on."""
    arrs, kw = lp.give_up_scene(name)
    n = len(arrs[0])
    assert lp.plan(n)["bfs"] == 1
    eng, ref = _pair(arrs, **kw)
    mir = bh_amd.Engine(eng.params, device=0)
    ref2 = oracle.Oracle(*arrs, **kw)
    try:
        if name.startswith("pairs"):
            eng.compute_accelerations()  # (on a copy of the start: _evaluate builds afresh)
            assert eng.last_tree_nodes() > lp.plan(n)["bfs_bits"]
            eng.reset_bodies(*arrs)
        _evaluate(eng, ref)
        eng.reset_bodies(*arrs)
        ref.reset_bodies(*arrs)
        _advance(eng, ref, (3,))
        mir.reset_bodies(*arrs)
        mir.set_mirror(True)
        for f in range(3):
            mir.step(1)
            ref2.step(1)
            _assert_arrays_equal(mir.map_bodies(), ref2.get_bodies(), f"{name} frame {f}")
    finally:
        eng.close()
        mir.close()
        ref.close()
        ref2.close()


# ---- d. crossing the switches in one engine's life ---------------------------------------------

CROSS_FIELDS = ("small_front", "bfs", "kick_bpw")


def _cross_window():
    """(lowest, highest) size, within 64 bodies of the end of the small front, at which the small
    front, the breadth-first walk or the kick-only walk's bodies per wave switch."""
    front = lp.field_boundaries("small_front", 2, 70_000)[0]
    b = lp.boundaries(front - 64, front + 64, CROSS_FIELDS)
    return b[0], b[-1]


@functools.lru_cache(maxsize=None)
def _crossing_scene():
    """A heavy body at rest and three rings of 8 light bodies falling onto it at 1.5 px per
    step from 8.9, 10.4 and 11.9 px: one ring per step comes inside mergeMinDist = 8 (BHA:478).
    The list starts 13 bodies above the highest switch; every mass is distinct."""
    lo, hi = _cross_window()
    n0 = hi + 13
    rings = 24
    field = scenes.uniform(n0 - 1 - rings, 0.5, seed=31)
    hx, hy = 1200.37, 400.21
    away = (field[0] - hx) ** 2 + (field[1] - hy) ** 2 > 30.0 ** 2
    fx = np.where(away, field[0], field[0] + 60.0)  # (nobody else near the heavy)
    k = np.repeat(np.arange(1, 4), 8)
    phi = 2.0 * np.pi * np.tile(np.arange(8), 3) / 8.0 + 0.1 * k
    r = 8.0 + 1.5 * k - 0.6
    rx, ry = hx + r * np.cos(phi), hy + r * np.sin(phi)
    rvx, rvy = -300.0 * np.cos(phi), -300.0 * np.sin(phi)
    h = len(fx) // 2  # the heavy and its rings in the middle of the list
    x = np.concatenate([fx[:h], [hx], rx, fx[h:]])
    y = np.concatenate([field[1][:h], [hy], ry, field[1][h:]])
    vx = np.concatenate([field[2][:h], [0.0], rvx, field[2][h:]])
    vy = np.concatenate([field[3][:h], [0.0], rvy, field[3][h:]])
    m = 0.5 + 1e-6 * np.arange(n0)
    m[h] = 6000.0
    return x, y, vx, vy, m


@functools.lru_cache(maxsize=None)
def _crossing_counts():
    """The oracle's body count before and after each of the five steps."""
    ref = oracle.Oracle(*_crossing_scene(), theta=0.5)
    counts = [ref.num_bodies()]
    for _ in range(5):
        ref.step(1)
        counts.append(ref.num_bodies())
    ref.close()
    return counts


def _assert_crossing_inside_the_call():
    lo, hi = _cross_window()
    c = _crossing_counts()
    assert c[0] >= hi and c[1] >= hi, f"{c}: the call must start above every switch ({hi})"
    assert c[3] < lo, f"{c}: three steps must end below every switch ({lo})"
    assert c[0] - c[3] >= 20
    for f in CROSS_FIELDS:
        assert lp.plan(c[0])[f] != lp.plan(c[3])[f], f


@pytest.mark.parametrize("how", ["one_call", "one_step_calls", "async"])
def test_merges_cross_the_switches_mid_call(how):
    """N falls through the small-front, breadth-first and 4 -> 2 bodies-per-wave switches
    inside one step(5): the splitters, the lane map and the carried tree of the larger list meet
    the kernels of the smaller one.  Also as five one-step calls and as bh_step_begin /
    bh_step_end; the removed indices against the reference's."""
    _assert_crossing_inside_the_call()
    arrs = _crossing_scene()
    eng, ref = _pair(arrs, theta=0.5)
    try:
        if how == "one_call":
            _advance(eng, ref, (5,))
            want, _ = _removed_from_oracle(arrs, 5, theta=0.5)
            assert np.array_equal(eng.last_removed(), want)
        elif how == "one_step_calls":
            _advance(eng, ref, (1,) * 5)
        else:
            eng.set_mirror(True, buffers=2)
            removed = _async_call(eng, ref, 5, "crossing")
            assert removed == _crossing_counts()[0] - _crossing_counts()[5]
            want, _ = _removed_from_oracle(arrs, 5, theta=0.5)
            assert np.array_equal(eng.last_removed(), want)
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("mirror", [0, 2])
def test_one_engine_reused_across_the_switches(mirror):
    """One engine through bh_reset_bodies above, below and on the switches, down to an empty
    list and up again (stale splitters and lane map, capacity kept and grown): after each reset
    an evaluation and two steps against a fresh oracle; once with the double-buffered mirror."""
    sf = lp.field_boundaries("small_front", 2, 70_000)[0]  # the first size beyond the front
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    if mirror:
        eng.set_mirror(True, buffers=mirror)
    try:
        for i, n in enumerate((70_000, 3_000, sf, 64, 0, 12_500, 70_000)):
            arrs = _ladder_scene(n, offset=37 * i) if n else tuple(np.zeros(0) for _ in range(5))
            eng.reset_bodies(*arrs)
            ref = oracle.Oracle(*arrs, theta=0.5)
            what = f"reset {i} to {n} bodies"
            for visits in (False, True):  # the production walk, then the counting walk
                got = eng.compute_accelerations(visits=visits)
                want = ref.accelerations(visits=visits)
                _assert_finite("accelerations", *want[:2])
                for g, w in zip(got[:2], want[:2]):
                    assert bits_equal(g, w), what
                if visits:
                    assert np.array_equal(got[2], want[2]), what
            _assert_state_equal(eng, ref)
            eng.step(2)
            ref.step(2)
            _assert_finite("state", *ref.get_bodies())
            _assert_state_equal(eng, ref)
            if mirror:
                _assert_arrays_equal(eng.map_bodies(), ref.get_bodies(), what)
            ref.close()
    finally:
        eng.close()


# ---- e. removal indices against the reference ---------------------------------------------------

def _removed_from_oracle(initial, k, **kw):
    """Indices (into `initial`, ascending) of the bodies the reference's merge rule removes
    during k steps, and the reference's state after them -- from the oracle alone.

    The rule keeps list order and changes masses only (BHA:478-520), at the end of a step.  So
    after one step every survivor has, bit for bit, the position and velocity the same body
    has after that step with the rule switched off (mergeMinDist = 0), and the survivors are
    found among those in order.  Light bodies keep their masses, all distinct at the start:
    every survivor that is not heavy must carry the initial mass of the index found for it.
    (The masses alone do not give the indices: where one heavy absorbs another, either could
    be the survivor with the grown mass.)"""
    m0 = np.asarray(initial[4])
    assert len(np.unique(m0)) == len(m0), "initial masses must be distinct"
    max_mass = kw.get("merge_max_mass", 4000.0)
    alive = np.arange(len(m0))
    state = tuple(np.array(a, dtype=np.float64) for a in initial)
    for _ in range(k):
        merged = oracle.Oracle(*state, **kw)
        merged.step(1)
        surv = merged.get_bodies()
        merged.close()
        free = oracle.Oracle(*state, **dict(kw, merge_min_dist=0.0))
        free.step(1)
        every = free.get_bodies()
        free.close()
        assert len(every[0]) == len(state[0])
        rows = np.stack([a.view(np.int64) for a in every[:4]], axis=1)
        srow = np.stack([a.view(np.int64) for a in surv[:4]], axis=1)
        keep, j = [], 0
        for i in range(len(rows)):
            if j < len(srow) and np.array_equal(rows[i], srow[j]):
                keep.append(i)
                j += 1
        assert j == len(srow), "a survivor is not among the step's bodies"
        alive = alive[np.array(keep, dtype=np.int64)]
        state = surv
    light = state[4] <= max_mass
    assert bits_equal(state[4][light], m0[alive][light]), "a light survivor changed its mass"
    assert np.all(state[4][~light] >= m0[alive][~light])
    return np.setdiff1d(np.arange(len(m0)), alive), state


def _merge_rule_scene():
    """test_merge_rule's bodies, every mass distinct."""
    bx = [1000.0, 1007.9, 1008.1, 1000.0, 1003.0, 1500.0, 1504.0, 1200.0, 1200.5]
    by = [400.0, 400.0, 400.0, 406.0, 403.0, 300.0, 300.0, 200.0, 200.0]
    bm = [5000.0, 1.0, 1.25, 2.0, 4500.0, 10.0, 9000.0, 3.0, 4001.0]
    field = scenes.uniform(300, 0.5, seed=9)
    fm = field[4] + 1e-6 * np.arange(1, 301)
    return (np.concatenate([bx, field[0]]), np.concatenate([by, field[1]]),
            np.concatenate([np.zeros(9), field[2]]), np.concatenate([np.zeros(9), field[3]]),
            np.concatenate([bm, fm]))


def _mailbox_scene():
    """test_merge_rule_more_pairs_than_the_mailbox's crowd of heavies, every mass distinct."""
    rng = np.random.default_rng(77)
    nh = 520
    hx = 1000.0 + 20.0 * rng.random(nh)
    hy = 400.0 + 20.0 * rng.random(nh)
    hm = rng.uniform(4001.0, 6000.0, nh)
    field = scenes.uniform(3000, 0.5, seed=17)
    x = np.concatenate([hx, field[0]])
    y = np.concatenate([hy, field[1]])
    m = np.concatenate([hm, field[4] + 1e-6 * np.arange(1, 3001)])
    perm = rng.permutation(len(x))
    arrs = tuple(a[perm] for a in (x, y, np.zeros(len(x)), np.zeros(len(x)), m))
    d2 = (hx[:, None] - x[None, :]) ** 2 + (hy[:, None] - y[None, :]) ** 2
    assert (d2 < 64.0).sum() - nh > max(65_536, 2 * len(x))  # the first step overflows
    return arrs


@pytest.mark.parametrize("scene,k,kw", [
    (_merge_rule_scene, 1, dict(theta=0.5, dt=0.0)),
    (_merge_rule_scene, 3, dict(theta=0.5)),
    (_mailbox_scene, 3, dict(theta=0.5)),
], ids=["merge_rule_dt0", "merge_rule_3_steps", "mailbox_overflow_replay"])
def test_removed_indices_match_the_reference(scene, k, kw):
    """bh_last_removed after one call of k steps = the indices the reference's rule removes,
    found from the oracle alone (not from the engine's own survivors)."""
    arrs = scene()
    want, state = _removed_from_oracle(arrs, k, **kw)
    assert len(want) > 0
    eng, ref = _pair(arrs, **kw)
    try:
        _advance(eng, ref, (k,))
        _assert_arrays_equal(ref.get_bodies(), state, "the oracle step by step")
        got = eng.last_removed()
        assert np.array_equal(got, want), (
            f"removed {len(got)} vs {len(want)}; first difference "
            f"{np.setxor1d(got, want)[:5]}")
    finally:
        eng.close()
        ref.close()
