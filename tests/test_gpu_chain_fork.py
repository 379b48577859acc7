"""The pipelined step's overlapped chain (merge rule, then the next step's first build) forks at
the end of the second build's k_emit_com and runs beside that build's spanning passes, the
traversal's input copies and the second traversal (engine.cpp evaluate_pipelined).  What the late
launch used to order for free is checked here against the CPU oracle, every fp64 word of every
field and the body counts:

  * the rule writes masses and flags only after the traversal's own copies of them exist -- also
    in the steps whose build leaves the copies to k_trav_inputs (a re-sorted lane map);
  * lastTree's walk buffers trade places between the span passes' launch and the overlapped
    build's, with and without the mirror, whether or not the call's last step merged;
  * a mailbox overflow replays the call only after the forked chain has ended;
  * dt = 0: the rule alone, its masses and its removals.

The scenes merge in most steps, and every case asserts that bodies were removed: none can pass
with the rule idle.  1025 bodies fill two emission chunks (one chunk boundary, spanning nodes),
3000 three.
"""
import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from conftest import bits_equal

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "vx", "vy", "m")
MERGE = dict(merge_max_mass=4000.0, merge_min_dist=8.0)
N_INFALL = 48


def _infall_scene(n, r0=8.02):
    """Two disks whose centres (50 000 and 5 000) are heavy, and 48 light bodies at rest relative
    to a centre, alternately around either, at radii r0 + 0.3 j: they cross mergeMinDist = 8 one
    after the other (a body at rest 8 from the large centre falls ~0.8 in one step), so the rule
    removes bodies in most steps.  List order shuffled, every mass distinct."""
    n2 = (n - N_INFALL) // 5
    d = scenes.two_disks(n - N_INFALL - n2, n2)
    heavy = np.flatnonzero(d[4] > MERGE["merge_max_mass"])
    assert len(heavy) == 2
    rng = np.random.default_rng(n)
    k = np.arange(N_INFALL)
    c = heavy[k % 2]
    r = r0 + 0.30 * (k // 2)
    phi = 2 * np.pi * rng.random(N_INFALL)
    extra = (d[0][c] + r * np.cos(phi), d[1][c] + r * np.sin(phi), d[2][c].copy(), d[3][c].copy(),
             np.full(N_INFALL, 0.5))
    arrs = tuple(np.concatenate([a, b]) for a, b in zip(d, extra))
    perm = rng.permutation(n)
    arrs = tuple(a[perm] for a in arrs)
    return arrs[:4] + (arrs[4] + 1e-6 * np.arange(1, n + 1),)


def _assert_arrays_equal(got, want, what):
    assert len(got[0]) == len(want[0]), f"{what}: N {len(got[0])} vs {len(want[0])}"
    for k, name in enumerate(FIELDS):
        bad = np.flatnonzero(np.asarray(got[k]).view(np.int64) != want[k].view(np.int64))
        assert bad.size == 0, f"{what} {name}: {bad.size} words differ, first at {bad[:5]}"


def _assert_quads_equal(eng, ref, what):
    for u, v in zip(eng.get_quads(), ref.quads()):
        assert bits_equal(u, v), f"{what}: quads"


@pytest.mark.parametrize("n", [1025, 3000])
def test_one_call_of_7_steps_against_7_calls_against_the_oracle(n):
    """Seven steps cross two lane-map refreshes (every third build) in steps that also merge."""
    arrs = _infall_scene(n)
    p = bh_amd.default_params(theta=0.5, **MERGE)
    one, many = bh_amd.Engine(p), bh_amd.Engine(p)
    ref = oracle.Oracle(*arrs, theta=0.5, **MERGE)
    try:
        one.reset_bodies(*arrs)
        many.reset_bodies(*arrs)
        one.step(7)
        for s in range(7):
            many.step(1)
            ref.step(1)
            _assert_arrays_equal(many.get_bodies(), ref.get_bodies(), f"one-step call {s}")
        assert ref.num_bodies() < n - 7  # more removals than steps
        assert one.num_bodies() == many.num_bodies() == ref.num_bodies()
        _assert_arrays_equal(one.get_bodies(), ref.get_bodies(), "the 7-step call")
        assert len(one.last_removed()) == n - ref.num_bodies()
        _assert_quads_equal(one, ref, "the 7-step call")
        # (a fresh tree after a merging last step jitters the bodies, BHA:146-151)
        _assert_arrays_equal(one.get_bodies(), ref.get_bodies(), "after the quads")
        one.step(2)  # the carried tree of a call whose chain forked, consumed by the next call
        ref.step(2)
        _assert_arrays_equal(one.get_bodies(), ref.get_bodies(), "the call after")
    finally:
        one.close()
        many.close()
        ref.close()


@pytest.mark.parametrize("n", [1025, 3000])
def test_mirror_and_last_tree_after_merging_and_quiet_last_steps(n):
    """Calls of 1 to 3 steps, with the mirror (its last step runs the rule in line, before the
    mirror's gathers) and without (the forked chain, lastTree's buffers traded under it); the
    quads after every call -- after calls whose last step merged and after calls whose last step
    did not, both of which must occur."""
    arrs = _infall_scene(n)
    p = bh_amd.default_params(theta=0.5, **MERGE)
    eng, mir = bh_amd.Engine(p), bh_amd.Engine(p)
    ref = oracle.Oracle(*arrs, theta=0.5, **MERGE)
    try:
        eng.reset_bodies(*arrs)
        mir.reset_bodies(*arrs)
        mir.set_mirror(True)
        merged_last, quiet_last = 0, 0
        for c, k in enumerate((3, 1, 2, 3, 2, 1, 3, 3, 2, 3)):
            eng.step(k)
            mir.step(k)
            ref.step(k - 1)
            before = ref.num_bodies()
            ref.step(1)
            if ref.num_bodies() < before:
                merged_last += 1
            else:
                quiet_last += 1
            want = ref.get_bodies()
            _assert_arrays_equal(mir.map_bodies(), want, f"call {c} mirror")
            _assert_arrays_equal(eng.get_bodies(), want, f"call {c}")
            for e, what in ((eng, f"call {c}"), (mir, f"call {c} mirror")):
                _assert_quads_equal(e, ref, what)
            want = ref.get_bodies()
            _assert_arrays_equal(mir.map_bodies(), want, f"call {c} mirror after the quads")
            _assert_arrays_equal(eng.get_bodies(), want, f"call {c} after the quads")
        assert merged_last >= 2 and quiet_last >= 2, (merged_last, quiet_last)
        assert eng.num_bodies() == mir.num_bodies() == ref.num_bodies() < n
    finally:
        eng.close()
        mir.close()
        ref.close()


def test_mailbox_overflow_replays_a_3_step_call():
    """520 heavy bodies within a 20 x 20 box among 3000 light ones: ~9e4 candidate pairs in the
    first step against a mailbox of max(65 536, 2 N).  The overflow is seen at the end of the
    call, after the forked chains of all three steps; the call is replayed with a larger mailbox
    (reallocated with no chain in flight) and equals the oracle; so does the call after it."""
    rng = np.random.default_rng(78)
    nh = 520
    hx = 1000.0 + 20.0 * rng.random(nh)
    hy = 400.0 + 20.0 * rng.random(nh)
    hm = rng.uniform(4001.0, 6000.0, nh)
    field = scenes.uniform(3000, 0.5, seed=18)
    x = np.concatenate([hx, field[0]])
    y = np.concatenate([hy, field[1]])
    m = np.concatenate([hm, field[4]])
    perm = rng.permutation(len(x))
    arrs = tuple(a[perm] for a in (x, y, np.zeros(len(x)), np.zeros(len(x)), m))
    d2 = (hx[:, None] - x[None, :]) ** 2 + (hy[:, None] - y[None, :]) ** 2
    assert (d2 < 64.0).sum() - nh > max(65_536, 2 * len(x))  # the first step overflows
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5, **MERGE))
    ref = oracle.Oracle(*arrs, theta=0.5, **MERGE)
    try:
        eng.reset_bodies(*arrs)
        eng.step(3)
        ref.step(3)
        _assert_arrays_equal(eng.get_bodies(), ref.get_bodies(), "the replayed call")
        assert eng.num_bodies() < len(x) - nh // 2
        assert len(eng.last_removed()) == len(x) - eng.num_bodies()
        eng.step(2)
        ref.step(2)
        _assert_arrays_equal(eng.get_bodies(), ref.get_bodies(), "the call after")
    finally:
        eng.close()
        ref.close()


def _removed_from_oracle(initial, k, **kw):
    """Indices (into `initial`, ascending) the reference's rule removes during k steps, from the
    oracle alone: the rule keeps list order and changes masses only (BHA:478-520), so a step's
    survivors are found, in order and bit for bit in position and velocity, among the bodies of
    the same step with the rule off (mergeMinDist = 0)."""
    alive = np.arange(len(initial[0]))
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
    return np.setdiff1d(np.arange(len(initial[0])), alive), state


@pytest.mark.parametrize("n", [1025, 3000])
def test_dt_zero_masses_and_removal_order(n):
    """Positions fixed: the infall bodies start at radii from 6.5, several of them inside
    mergeMinDist of either centre, and a 4500 body lies 3 from the large centre (a heavy
    victim).  Three steps in one call: the masses, and bh_last_removed against the removals
    found from the oracle alone."""
    arrs = _infall_scene(n, r0=6.5)
    big = int(np.argmax(arrs[4]))
    near = int(np.argmin(arrs[4]))
    arrs[0][near], arrs[1][near] = arrs[0][big] + 3.0, arrs[1][big]
    arrs[2][near], arrs[3][near] = arrs[2][big], arrs[3][big]
    arrs[4][near] = 4500.0
    kw = dict(theta=0.5, dt=0.0, **MERGE)
    want, state = _removed_from_oracle(arrs, 3, **kw)
    # (whichever of the two heavies is first in the list absorbs the other, BHA:478-520)
    assert len(want) >= 8 and (near in want) != (big in want)
    eng = bh_amd.Engine(bh_amd.default_params(**kw))
    ref = oracle.Oracle(*arrs, **kw)
    try:
        eng.reset_bodies(*arrs)
        eng.step(3)
        ref.step(3)
        _assert_arrays_equal(ref.get_bodies(), state, "the oracle step by step")
        _assert_arrays_equal(eng.get_bodies(), ref.get_bodies(), "dt = 0")
        assert eng.num_bodies() == n - len(want)
        got = eng.last_removed()
        assert np.array_equal(got, want), (
            f"removed {len(got)} vs {len(want)}; first difference {np.setxor1d(got, want)[:5]}")
    finally:
        eng.close()
        ref.close()
