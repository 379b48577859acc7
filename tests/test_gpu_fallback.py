"""GPU: the IEEE fallback branches of the force and potential kernels, and fp32 nbody3d's edges.

k_traverse, k_direct, k_direct_potential and the potential walk take their exact reduced-range
sequences (FAST) only while fast_s2_ok, lane_fast_ok and lane_self_ok hold for the whole wave
(csrc/fastmath.hpp): soft2 in [2^-600, 2^500], |x|, |y| < 2^32, |G m^2| < 2^400.  The other
GPU tests stay inside those guards, but for the waves that hold a NaN body of the zero-mass
scenes.  Here soft2, theta, G, dt, far-flung and heavy bodies sit on
and beyond them, so the FAST = false instantiations run: full IEEE sqrt and divide, the own leaf
skipped by identity, NODE_SKIP tested, the ldexp form of the opening criterion.

Rule of every fp64 comparison: the oracle's own accelerations and state are asserted finite
first, then every word is compared bit for bit (no equal_nan); the one case that is NaN by
construction asserts which entries are not finite.  tests/test_oracle.py pins the C oracle to
the independent Python restatement on the same parameters.

nbody3d (fp32) is measured against the fp64 restatement of the shader (oracle/py_gpu3d.py) on
inputs whose coordinate differences are exact in fp32, within the summation bound
(n + 16) 2^-24 sum_j |t_ij| per body and component: n roundings of the running sum and 16 for
the roundings of one term (three fma of r2, the 1-ulp v_rsq_f32 = 2 units, cubed: 12.5; G m,
its product with invR^3 and the product with d: 15.5).
"""
import functools

import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from oracle import py_gpu3d
from test_gpu_parity import (FIELDS, _assert_acc_equal, _assert_arrays_equal, _assert_state_equal,
                             _pair, _production_walk, _run_group)
from test_gpu_potential import _assert_bits, _assert_sums, _check_phi, _engine, _terms
from test_oracle import (DT_EDGES, G_EDGES, HEAVY_MASSES, P500, P600, THETA_EDGES,
                         coincident_pair, massless_cells_scene, with_far_bodies, with_guard_bodies,
                         with_heavy_body)
from test_potential_ref import checker_phi, make_cfg, theta0_phi

pytestmark = pytest.mark.gpu

INF = float("inf")
# both sides of each guard of lane_fast_ok, the smallest subnormal, and far beyond
SOFT2 = [0.0, 5e-324, float(np.nextafter(P600, 0.0)), P600, P500, float(np.nextafter(P500, INF)),
         1e200, INF]
HEAVY_MODES = {"walk_nomerge": dict(theta=0.5, merge_min_dist=0.0),
               "walk_merge": dict(theta=0.5),
               "direct_nomerge": dict(theta=0.0, merge_min_dist=0.0)}
HEAVY_AT = 1234  # a satellite of the large disk


@functools.lru_cache(maxsize=None)
def _small():
    """3200 bodies (n <= 4096: the breadth-first kernel walks first), one coincident pair."""
    return coincident_pair(scenes.two_disks(2500, 700), 900, 2900)


@functools.lru_cache(maxsize=None)
def _medium():
    """6000 bodies: the cursor walk with fewer than 64 bodies per wave."""
    return scenes.two_disks(4600, 1400)


@functools.lru_cache(maxsize=None)
def _large():
    """66 000 bodies: full 64-body waves, so a slow lane takes 63 ordinary bodies along."""
    return scenes.kepler_disk(66_000)


def _copy(arrs):
    return tuple(a.copy() for a in arrs)


def _assert_finite(what, *arrays):
    for a in arrays:
        assert np.all(np.isfinite(a)), f"the oracle's {what} is not finite"


def _evaluate(eng, ref):
    """_assert_acc_equal with the oracle's finiteness asserted before any comparison: the
    production walk (theta = 0: k_direct), the counting walk, the visit counts and the state
    after the build's jitter, bit for bit."""
    rax, ray, rvis = ref.accelerations(visits=True)
    _assert_finite("accelerations", rax, ray)
    _assert_finite("state after the build", *ref.get_bodies())
    fx, fy = _production_walk(eng)
    ax, ay, vis = eng.compute_accelerations(visits=True)
    _assert_bits(fx, rax, "production walk ax")
    _assert_bits(fy, ray, "production walk ay")
    _assert_bits(ax, rax, "counting walk ax")
    _assert_bits(ay, ray, "counting walk ay")
    assert np.array_equal(vis, rvis), "node-visit counts differ"
    _assert_state_equal(eng, ref)


def _advance(eng, ref, calls=(3,)):
    for k in calls:
        eng.step(k)
        ref.step(k)
    _assert_finite("state", *ref.get_bodies())
    _assert_state_equal(eng, ref)


def _check(arrs, calls=(3,), **kw):
    eng, ref = _pair(_copy(arrs), **kw)
    try:
        _evaluate(eng, ref)
        _advance(eng, ref, calls)
    finally:
        eng.close()
        ref.close()


# ---- B. fp64 forces against the C oracle ----------------------------------------------------

@pytest.mark.parametrize("theta", [0.5, 0.0])
@pytest.mark.parametrize("soft2", SOFT2, ids=repr)
def test_soft2_edges(soft2, theta):
    """Config.SOFTENING is a var: 0 and anything outside [2^-600, 2^500] sends every wave of
    the walks (theta 0.5) and of k_direct (theta 0) down the fallback; the values at the
    guards themselves stay on the fast path.  Both sides must match."""
    _check(_small(), theta=theta, soft2=soft2)


@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_soft2_zero_in_one_step_calls(theta):
    """One-step calls carry the tree from call to call (the pipelined path) instead of
    building inside one call."""
    _check(_small(), calls=(1, 1, 1), theta=theta, soft2=0.0)


@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_far_bodies(theta):
    """|x| = 2^250, nextafter(2^250, 0) and 1e100, y = 1e200 and -1e160 at list indices 0,
    n/4, n/2, 3n/4 and last: outside the root cell, so never in the tree, but walked, kicked
    and drifted, and the drift's fused Morton key sees their coordinates.  All lie beyond
    lane_fast_ok's position bound; at theta 0.5 and this size each is alone in its wave (the
    breadth-first launch shape), at theta 0 they share k_direct's tail wave with ordinary
    bodies.  nextafter(2^250, 0) has a significand of all ones, which every node's r copies:
    the divisor that only the IEEE reciprocal rounds correctly (csrc/fastmath.hpp)."""
    arrs = with_far_bodies(_small())
    assert abs(arrs[0][0]) == 1e100 and abs(arrs[1][-1]) == 1e160
    _check(arrs, theta=theta)


@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_bodies_on_both_sides_of_the_position_guard(theta):
    """|x|, |y| against 2^32 (lane_fast_ok): -2^32, y = 2^32 and x = nextafter(2^64, 0) walk
    the fallback; 3 * 2^30 and the all-ones coordinates x = nextafter(2^32, 0) and
    y = -nextafter(2^32, 0) take the FAST sequences with d2 up to 2^64.  The all-ones
    significand is the one that matters: beyond the bound every node near the axis copies it
    into r, inside it no node of this scene does."""
    _check(with_guard_bodies(_small()), theta=theta)


@pytest.mark.parametrize("mode", list(HEAVY_MODES))
@pytest.mark.parametrize("mass", HEAVY_MASSES, ids=repr)
def test_heavy_body(mass, mode):
    """G m^2 against 2^400 (lane_self_ok): 1e59 is just inside, 1e61 just outside.  After the
    first step the heavy body has flung everything out of the root cell: the later steps run
    on an empty tree with every body outside."""
    _check(with_heavy_body(_small(), mass, HEAVY_AT), **HEAVY_MODES[mode])


def test_heavy_body_whose_centre_of_mass_overflows():
    """m = 1e306, the one non-finite case.  x * m overflows, so the root's centre of mass is
    inf / 1e306 = inf; for every body dx = inf, d2 = inf, the root is accepted (s2 < inf) and
    its term is f * dx * invR = 0 * inf * 0 = NaN: every acceleration is NaN, and after a step
    every position and velocity, while the masses stay as they were.  Exactly that set is
    asserted on the oracle and on the engine before the words are compared with equal_nan."""
    arrs = with_heavy_body(_small(), 1e306, HEAVY_AT)
    eng, ref = _pair(_copy(arrs), theta=0.5, merge_min_dist=0.0)
    twin = oracle.Oracle(*_copy(arrs), theta=0.5, merge_min_dist=0.0)
    rax, ray = twin.accelerations()
    twin.close()
    try:
        assert np.all(np.isnan(rax)) and np.all(np.isnan(ray))
        fx, fy = _production_walk(eng)
        assert np.all(np.isnan(fx)) and np.all(np.isnan(fy))
        _assert_acc_equal(eng, ref, nan_ok=True)
        eng.step(3)
        ref.step(3)
        got, want = eng.get_bodies(), ref.get_bodies()
        for name, g, w in zip(FIELDS, got, want):
            assert np.isnan(g).sum() == np.isnan(w).sum() == (0 if name == "m" else len(w)), name
        _assert_bits(got[4], arrs[4], "m")
        _assert_state_equal(eng, ref, nan_ok=True)
    finally:
        eng.close()
        ref.close()


def test_massless_cells_on_the_fallback():
    """NODE_SKIP in the fallback walk: cells of negative-mass bodies only have mass 0 and the
    reference returns there (BHA:216).  Taken as a node instead, a massless cell adds
    G m * 0 / r2 -- an exact zero that no finite result shows, unless r2 = 0: with soft2 = 0,
    the body at (0, 0) and the negative body at a massless cell's centre sit exactly where the
    builds record such a cell (0, 0 or the cell centre), and the term is 0 * inf = NaN."""
    _check(massless_cells_scene(3000), theta=0.5, soft2=0.0)


@pytest.mark.parametrize("G", G_EDGES, ids=repr)
def test_G_edges(G):
    """G = 0 (every force +-0), negative, and 1e200 (G m^2 beyond lane_self_ok for every body)."""
    _check(_small(), theta=0.5, G=G)


@pytest.mark.parametrize("dt", DT_EDGES, ids=repr)
def test_dt_edges(dt):
    _check(_small(), theta=0.5, dt=dt)


@pytest.mark.parametrize("theta", THETA_EDGES, ids=repr)
def test_theta_edges(theta):
    """Negative theta (theta^2 is what the criterion uses), -0.0, 1e-200 whose square
    underflows to zero -- the step is pipelined and lane-mapped (theta != 0) yet runs k_direct
    (theta^2 == 0) --, 1e-160 whose square is subnormal, 1e160 and inf whose square is inf."""
    _check(_small(), theta=theta)


def test_theta_squared_underflow_in_one_step_calls_with_the_mirror():
    eng, ref = _pair(_copy(_small()), theta=1e-200)
    try:
        eng.set_mirror(True)
        for f in range(3):
            eng.step(1)
            ref.step(1)
            want = ref.get_bodies()
            _assert_finite("state", *want)
            _assert_arrays_equal(eng.map_bodies(), want, f"call {f} mirror")
            _assert_arrays_equal(eng.get_bodies(), want, f"call {f}")
    finally:
        eng.close()
        ref.close()


def test_live_soft2_change_across_the_guard():
    """soft2 1 -> 0 -> 1 between calls on one engine: forces cached for the next step must not
    survive the change."""
    eng, ref = _pair(_copy(_small()), theta=0.5)
    try:
        for soft2 in (1.0, 0.0, 1.0):
            eng.set_params(bh_amd.default_params(theta=0.5, soft2=soft2))
            ref.set_params(oracle.params(theta=0.5, soft2=soft2))
            eng.step(2)
            ref.step(2)
            _assert_finite("state", *ref.get_bodies())
            _assert_state_equal(eng, ref)
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("case", ["soft2_0", "far", "heavy"])
@pytest.mark.parametrize("size", ["medium", "large"])
def test_fallback_at_the_larger_launch_shapes(size, case):
    """The launch shape follows n: 6000 bodies take the cursor walk with short waves, 66 000
    the production shape (full waves, 8 per workgroup, wave ordering), the only one where a
    slow lane drags 63 ordinary bodies through the fallback.  One evaluation and step(2)."""
    arrs = _medium() if size == "medium" else _large()
    kw = dict(theta=0.5)
    if case == "soft2_0":
        kw["soft2"] = 0.0
    elif case == "far":
        arrs = with_far_bodies(arrs)
    else:
        arrs = with_heavy_body(arrs, 1e61, len(arrs[0]) // 3)
    _check(arrs, calls=(2,), **kw)


@pytest.mark.parametrize("case", ["soft2_0", "soft2_1e200", "far_and_heavy"])
@pytest.mark.parametrize("let", ["default", "0"])
def test_multi_rank_on_the_fallback(let, case, monkeypatch):
    """Two ranks in one process, locally essential trees and BH_LET=0: let_include_gap2 with a
    negative or infinite radicand, and the KICK_OWN_* variants behind the fallback walk.
    Every rank's state after step(3) equals the oracle's."""
    if let == "0":
        monkeypatch.setenv("BH_LET", "0")
    else:
        monkeypatch.delenv("BH_LET", raising=False)
    arrs, kw = scenes.config_scene("c1_code"), dict(theta=0.5)
    if case == "soft2_0":
        kw["soft2"] = 0.0
    elif case == "soft2_1e200":
        kw["soft2"] = 1e200
    else:
        arrs = with_heavy_body(with_far_bodies(arrs), 1e61, 5000)
    ref = oracle.Oracle(*_copy(arrs), **kw)
    ref.step(3)
    want = ref.get_bodies()
    ref.close()
    _assert_finite("state", *want)
    results, _ = _run_group(2, bh_amd.default_params(**kw), _copy(arrs), (3,))
    for r in range(2):
        _assert_arrays_equal(results[r], want, f"rank {r}")


# ---- C. the potential against the Python checkers -------------------------------------------

PHI_SOFT2 = [0.0, float(np.nextafter(P600, 0.0)), P500, float(np.nextafter(P500, INF))]


def _finite(reference):
    """`reference` with its phi asserted finite: _check_phi compares words, and a NaN on both
    sides would agree with itself."""
    def checked(arrs, cfg):
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            phi, st = reference(arrs, cfg)
        _assert_finite("phi", phi)
        return phi, st
    return checked


def _phi_case(theta, far=False, **over):
    """theta 0.5: the potential walk against checker_phi; theta 0: the tiled all-pairs kernel
    (2100 leaves cross two 1024-leaf tiles) against theta0_phi.  Finite, then bit for bit."""
    arrs = scenes.two_disks(1500, 500) if theta else scenes.two_disks(1600, 500)
    if far:
        arrs = with_far_bodies(arrs)
    cfg = make_cfg(theta=theta, **over)
    return _check_phi(arrs, cfg, reference=_finite(checker_phi if theta else theta0_phi))


@pytest.mark.parametrize("theta", [0.5, 0.0])
@pytest.mark.parametrize("soft2", PHI_SOFT2, ids=repr)
def test_potential_soft2_edges(soft2, theta):
    _phi_case(theta, soft2=soft2)


@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_potential_far_bodies(theta):
    """The body at x = 1e100 (list index 0) still feels the tree; for y = 1e200 and -1e160 (the
    last two inserted, the second at the end) dy * dy overflows, r2 = inf and 1 / sqrt(r2) = 0."""
    phi = _phi_case(theta, far=True)
    base = len(phi) - 5
    assert phi[0] < 0.0
    assert phi[3 * base // 4 + 3] == 0.0 and phi[-1] == 0.0


def test_potential_massless_cells_on_the_fallback():
    """NODE_SKIP in the fallback potential walk, as test_massless_cells_on_the_fallback."""
    arrs, cfg = massless_cells_scene(2000), make_cfg(theta=0.5, soft2=0.0)
    _check_phi(arrs, cfg, reference=_finite(checker_phi))


def test_potential_theta0_one_full_tile_soft2_zero():
    arrs = scenes.two_disks(800, 224)  # 1024 leaves fill one tile exactly
    cfg = make_cfg(theta=0.0, soft2=0.0)
    _check_phi(arrs, cfg, reference=_finite(theta0_phi))


def test_diagnostics_with_potential_at_soft2_zero():
    arrs, cfg = scenes.two_disks(1500, 500), make_cfg(theta=0.5, soft2=0.0)
    eng = _engine(arrs, cfg)
    try:
        d = eng.diagnostics(potential=True)
        phi, st = checker_phi(arrs, cfg)
        _assert_finite("phi", phi)
        for name, a, b in zip(FIELDS, eng.get_bodies(), st):
            _assert_bits(a, b, name)
        assert d.n == len(phi)
        _assert_sums(d, _terms(st, phi))
    finally:
        eng.close()


# ---- D. fp32 nbody3d against the fp64 restatement -------------------------------------------

U32 = 2.0 ** -24
N3D = [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def _grid_bodies(n, planar=False):
    """n distinct bodies on the 2^-8 grid within [-64, 64]^3 (every coordinate difference is
    exact in fp32), at rest or slow; masses in [0.5, 2] and one of 1e4 (body 0, n > 1); body
    n // 2 sits exactly at the origin, where the tile's pads are."""
    rng = np.random.default_rng(1000 + n)
    k = rng.integers(-64 * 256, 64 * 256 + 1, size=(4 * n + 8, 3))
    k = k[np.any(k != 0, axis=1)]
    _, first = np.unique(k, axis=0, return_index=True)
    k = k[np.sort(first)][:n].astype(np.float64)
    assert len(k) == n
    k[n // 2] = 0.0
    pos = k / 256.0
    if planar:
        pos[:, 2] = 0.0
        assert len(np.unique(pos, axis=0)) == n
    vel = rng.integers(-512, 513, size=(n, 3)) / 256.0
    m = rng.integers(128, 513, size=n) / 256.0
    if n > 1:
        m[0] = 1e4
    out = tuple(np.ascontiguousarray(c) for c in (*pos.T, *vel.T, m))
    for a in out:
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
        a.flags.writeable = False
    return out


def _check_acc3d(sim, arrs, softening, what):
    """accelerations of `sim` within (n + 16) 2^-24 sum_j |t_ij|; returns max error / bound."""
    x, y, z, _, _, _, m = arrs
    n = len(x)
    got = sim.accelerations(G=80.0, softening=softening)
    want, mag = py_gpu3d.accelerations_and_term_sums(x, y, z, m, G=80.0, softening=softening)
    with np.errstate(divide="ignore"):  # (softening 0: the excluded diagonal is 1 / 0)
        plain = py_gpu3d.accelerations(x, y, z, m, G=80.0, softening=softening)
    worst = 0.0
    for g, w, s, p in zip(got, want, mag, plain):
        assert np.all(np.isfinite(w)) and np.array_equal(w, p)
        assert np.all(np.isfinite(g)), f"{what}: {np.count_nonzero(~np.isfinite(g))} of {n} not finite"
        bound = (n + 16) * U32 * s
        err = np.abs(g.astype(np.float64) - w)
        if n > 1:
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        assert np.all(err <= bound), f"{what}: error / bound up to {np.max(err / np.maximum(bound, 1e-300)):.3f}"
    print(f"nbody3d {what}: max error / bound = {worst:.4f}")
    return got


@pytest.mark.parametrize("softening", [1.0, 0.0])
@pytest.mark.parametrize("n", N3D)
def test_nbody3d_sizes_and_softening_zero(n, softening):
    """Below one workgroup (256) and one tile (1024), at both exactly, one past (the last body
    in a packed pair's even slot with a pad beside it), self in the second and third tile; a
    body at the origin, where the pads sit.  With softening 0 the excluded self slot and the
    pads have r2 = 0: they must add exactly zero, as the shader's index test does (GPU.kt:134)."""
    arrs = _grid_bodies(n)
    sim = bh_amd.NBody3D(device=0)
    sim.set(*arrs)
    got = _check_acc3d(sim, arrs, softening, f"n={n} softening={softening}")
    if n == 1:
        assert all(g[0] == 0.0 for g in got)
    sim.close()


@pytest.mark.parametrize("softening", [1.0, 0.0])
def test_nbody3d_planar_input_has_no_z_force(softening):
    arrs = _grid_bodies(1025, planar=True)
    sim = bh_amd.NBody3D(device=0)
    sim.set(*arrs)
    got = _check_acc3d(sim, arrs, softening, f"planar softening={softening}")
    assert np.all(got[2] == 0.0)
    sim.close()


def _step_bounds(arrs, k, dt):
    """The fp64 restatement's state after k steps and first-order bounds of the fp32 engine's
    position and velocity error against it, per body (the largest component).

    Per step, with E the largest position error of any body so far:
      error of a   <= (n + 16) 2^-24 sum_j |t_ij|  +  2 E sum_j G m_j 4 / r_ij^3
                      (the kernel's own rounding; both ends of d_ij moved by up to E, and the
                      Jacobian of d / r^3 has eigenvalues in [-2, 1] / r^3: 4 covers the change
                      from the 2-norm to one component)
      error of v'  <= error of v + dt error of a + 2^-24 (|v'| + 2 |a dt|)     (a dt, the sum)
      error of x'  <= error of x + dt error of v' + 2^-24 (|x'| + 2 |v' dt|)
    """
    x, y, z, vx, vy, vz, m = (np.array(a, dtype=np.float64) for a in arrs)
    n = len(x)
    ex = np.zeros(n)
    ev = np.zeros(n)
    for _ in range(k):
        acc, mag = py_gpu3d.accelerations_and_term_sums(x, y, z, m, G=80.0, softening=1.0)
        r2 = ((x[None, :] - x[:, None]) ** 2 + (y[None, :] - y[:, None]) ** 2 +
              (z[None, :] - z[:, None]) ** 2 + 1.0)
        lip = 80.0 * m[None, :] * 4.0 / r2 ** 1.5
        np.fill_diagonal(lip, 0.0)
        ea = (n + 16) * U32 * np.max(mag, axis=0) + 2.0 * ex.max() * lip.sum(axis=1)
        a_abs = np.max(np.abs(acc), axis=0)
        vx, vy, vz = vx + acc[0] * dt, vy + acc[1] * dt, vz + acc[2] * dt
        x, y, z = x + vx * dt, y + vy * dt, z + vz * dt
        v_abs = np.max(np.abs([vx, vy, vz]), axis=0)
        x_abs = np.max(np.abs([x, y, z]), axis=0)
        ev = ev + dt * ea + U32 * (v_abs + 2.0 * a_abs * dt)
        ex = ex + dt * ev + U32 * (x_abs + 2.0 * v_abs * dt)
    return (x, y, z, vx, vy, vz, m), ex, ev


def test_nbody3d_steps_reuse_and_empty_set():
    """step(k) for k = 1, 2, 3 at n = 1025 (both parities of the double buffer, read through
    get), then a smaller list on the same handle, then an empty one.

    Positions and velocities against the fp64 restatement within twice the first-order bound
    of _step_bounds: the factor 2 is the margin for what first order leaves out (the bound's
    own terms are taken at the restatement's positions, not at the engine's, and products of
    two errors are dropped); dt = 2^-8 and softening = 1 keep those far below the bound."""
    dt = 2.0 ** -8
    arrs = _grid_bodies(1025)
    sim = bh_amd.NBody3D(device=0)
    for k in (1, 2, 3):
        sim.set(*arrs)
        sim.step(k, dt=dt, G=80.0, softening=1.0)
        got = sim.get()
        want, ex, ev = _step_bounds(arrs, k, dt)
        ref_step = py_gpu3d.step(*arrs, k=k, dt=dt, G=80.0, softening=1.0)
        for a, b in zip(want, ref_step):
            assert np.array_equal(a, b)  # _step_bounds advances as the restatement does
        perr = np.max([np.abs(got[c].astype(np.float64) - want[c]) for c in range(3)], axis=0)
        verr = np.max([np.abs(got[c].astype(np.float64) - want[c]) for c in range(3, 6)], axis=0)
        print(f"nbody3d step({k}): max position error / bound = {np.max(perr / ex):.4f}, "
              f"velocity {np.max(verr / ev):.4f} (allowed 2)")
        assert np.all(perr <= 2.0 * ex), np.max(perr / ex)
        assert np.all(verr <= 2.0 * ev), np.max(verr / ev)
        assert np.array_equal(got[6], np.float32(arrs[6]))
    # a smaller list within the old capacity: the buffers' tails hold stale bodies
    small = _grid_bodies(257)
    sim.set(*small)
    _check_acc3d(sim, small, 1.0, "n=257 after 1025")
    _check_acc3d(sim, small, 0.0, "n=257 after 1025, softening 0")
    for a, b in zip(sim.get(), small):
        assert np.array_equal(a, np.float32(b))
    # an empty list: every call succeeds on nothing
    sim.set(*[np.zeros(0, dtype=np.float32)] * 7)
    sim.step(2, dt=dt, G=80.0, softening=1.0)
    assert all(len(a) == 0 for a in sim.accelerations(G=80.0, softening=0.0))
    assert all(len(a) == 0 for a in sim.get())
    assert sim.center_of_mass_sums() == (0.0, 0.0, 0.0, 0.0)
    assert sim.center_of_mass() == (0.0, 0.0, 0.0)
    sim.close()
