"""GPU: bh_compute_potential / bh_compute_diagnostics / bh_nbody3d_center_of_mass.

Every phi check is bit-exact against the Python checker of tests/test_potential_ref.py built
from the same start state (the walk visits accumulateForce's nodes and adds mass / sqrt(r2) in
pre-order); the global sums are checked against math.fsum over numpy-computed terms within the
any-order summation bound (N + 16) 2^-53 sum|t_i|.
"""
import math
import os

import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from conftest import bits_equal
from test_potential_ref import (cfg_from_golden, checker_phi, energy, make_cfg, params_of,
                                sum_bound, theta0_phi)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("x", "y", "vx", "vy", "m")


def _engine(arrs, cfg, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    return eng


def _assert_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {bad[:5]}: "
                           f"{got[bad[:3]]} vs {want[bad[:3]]}")


def _check_phi(arrs, cfg, reference=checker_phi):
    """Engine phi and the state after the call against the checker's, bit for bit."""
    eng = _engine(arrs, cfg)
    phi = eng.compute_potential()
    want, st = reference(arrs, cfg)
    _assert_bits(phi, want, "phi")
    for name, a, b in zip(FIELDS, eng.get_bodies(), st):
        _assert_bits(a, b, name)  # the build's jitter is part of the call
    eng.close()
    return phi


def _golden_start(name):
    z = np.load(os.path.join(GOLDEN, name))
    return tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z)


def test_two_bodies_known_answer():
    arrs = (np.array([100.0, 103.0]), np.array([100.0, 104.0]), np.zeros(2), np.zeros(2),
            np.array([1.0, 2.0]))
    phi = _check_phi(arrs, make_cfg(theta=0.5, G=80.0, soft2=1.0, merge_min_dist=0.0))
    np.testing.assert_allclose(phi, [-160.0 / math.sqrt(26.0), -80.0 / math.sqrt(26.0)],
                               rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("theta", [0.2, 0.5, 1.0, 1.6])
def test_theta_sweep(theta):
    _check_phi(scenes.two_disks(1500, 500), make_cfg(theta=theta))


@pytest.mark.parametrize("n", [1, 2, 63, 65, 130])
def test_small_sizes(n):
    arrs = tuple(a[:n].copy() for a in scenes.two_disks(100, 40))
    phi = _check_phi(arrs, make_cfg(theta=0.5))
    if n == 1:
        assert phi[0] == 0.0


@pytest.mark.parametrize("n1,n2", [(1600, 500), (800, 224)])
def test_theta0_all_pairs(n1, n2):
    """theta = 0 runs the LDS-tiled all-pairs kernel over the leaf sequence: 2100 leaves cross
    two 1024-leaf tiles, 1024 fill one exactly."""
    arrs = scenes.two_disks(n1, n2)
    assert len(arrs[0]) in (2100, 1024)
    _check_phi(arrs, make_cfg(theta=0.0), reference=theta0_phi)


def test_bodies_outside_the_root():
    arrs, cfg = _golden_start("outside_153.npz")
    root_h = max(cfg["width_px"], cfg["height_px"]) / 2.0 + 2.0
    outside = (np.abs(arrs[0] - cfg["width_px"] / 2.0) >= root_h) | \
              (np.abs(arrs[1] - cfg["height_px"] / 2.0) >= root_h)
    assert outside.any()
    phi = _check_phi(arrs, cfg)
    assert np.all(phi[outside] < 0.0)  # they are walked: they feel the tree


def test_jitter_scene_positions_and_phi():
    arrs, cfg = _golden_start("jitter_306.npz")
    eng = _engine(arrs, cfg)
    phi = eng.compute_potential()
    want, st = checker_phi(arrs, cfg)
    _assert_bits(phi, want, "phi")
    got = eng.get_bodies()
    _assert_bits(got[0], st[0], "x after the jitter")
    _assert_bits(got[1], st[1], "y after the jitter")
    assert not bits_equal(got[0], arrs[0])  # the scene does jitter
    eng.close()


def test_zero_mass_bodies():
    arrs = tuple(a.copy() for a in scenes.two_disks(600, 200))
    arrs[4][np.random.default_rng(3).choice(800, 20, replace=False)] = 0.0
    _check_phi(arrs, make_cfg(theta=0.5))
    _check_phi(arrs, make_cfg(theta=0.0), reference=theta0_phi)


def test_after_stepping():
    """After step(3) merges have shrunk N and the traversal's lane map is live."""
    arrs = scenes.config_scene("c1_baseline")
    cfg = make_cfg(theta=0.5)
    eng = _engine(arrs, cfg)
    eng.step(3)
    now = eng.get_bodies()
    phi = eng.compute_potential()
    want, st = checker_phi(now, cfg)
    _assert_bits(phi, want, "phi after step(3)")
    for name, a, b in zip(FIELDS, eng.get_bodies(), st):
        _assert_bits(a, b, name)
    eng.close()


def test_state_semantics_of_compute_accelerations():
    arrs = scenes.two_disks(1500, 500)
    cfg = make_cfg(theta=0.5)
    a, b = _engine(arrs, cfg), _engine(arrs, cfg)
    a.compute_potential()
    b.compute_accelerations()
    a.step(5)
    b.step(5)
    for name, u, v in zip(FIELDS, a.get_bodies(), b.get_bodies()):
        _assert_bits(u, v, name)
    a.close()
    b.close()


def test_diagnostics_leave_the_state_alone():
    arrs = scenes.two_disks(1500, 500)
    cfg = make_cfg(theta=0.5)
    a, b = _engine(arrs, cfg), _engine(arrs, cfg)
    for _ in range(5):
        a.step(1)
        a.diagnostics(potential=False)
        b.step(1)
    for name, u, v in zip(FIELDS, a.get_bodies(), b.get_bodies()):
        _assert_bits(u, v, name)
    a.close()
    b.close()


def _terms(state, phi=None):
    x, y, vx, vy, m = state
    t = {"mass": m, "mx": m * x, "my": m * y, "px": m * vx, "py": m * vy,
         "lz": m * (x * vy - y * vx), "kinetic": 0.5 * m * (vx * vx + vy * vy)}
    if phi is not None:
        t["potential"] = m * phi
    return t


def _assert_sums(d, terms):
    for name, t in terms.items():
        want = math.fsum(t.tolist())
        bound = sum_bound(t)
        if name == "potential":
            want, bound = 0.5 * want, 0.5 * bound
        got = getattr(d, name)
        print(f"{name}: got {got!r} want {want!r} |diff| {abs(got - want):.3e} bound {bound:.3e}")
        assert abs(got - want) <= bound, name


@pytest.mark.parametrize("scene", ["two_disks", "outside"])
def test_diagnostics_values(scene):
    if scene == "two_disks":
        arrs, cfg = scenes.two_disks(1500, 500), make_cfg(theta=0.5)
    else:  # out-of-root bodies are live bodies: they are in every sum
        arrs, cfg = _golden_start("outside_153.npz")
    eng = _engine(arrs, cfg)
    eng.step(2)
    state = eng.get_bodies()
    d = eng.diagnostics(potential=False)
    assert d.n == len(state[0]) and d.potential == 0.0
    _assert_sums(d, _terms(state))
    assert eng.diagnostics(potential=False) == d  # identical bits
    for name, u, v in zip(FIELDS, eng.get_bodies(), state):
        _assert_bits(u, v, name)
    # with the potential: against the engine's own (verified) phi on the same start
    other = _engine(state, cfg)
    phi = other.compute_potential()
    after = other.get_bodies()
    dp = eng.diagnostics(potential=True)
    _assert_sums(dp, _terms(after, phi))
    assert dp.energy == dp.kinetic + dp.potential and dp.momentum == (dp.px, dp.py)
    assert dp.com == (dp.mx / dp.mass, dp.my / dp.mass)
    # two fresh engines on the same list return identical bits
    e1, e2 = _engine(state, cfg), _engine(state, cfg)
    d1, d2 = e1.diagnostics(potential=True), e2.diagnostics(potential=True)
    assert d1 == d2 == dp
    for e in (eng, other, e1, e2):
        e.close()


def test_diagnostics_of_an_empty_list():
    empty = tuple(np.zeros(0) for _ in range(5))
    eng = _engine(empty, make_cfg(theta=0.5))
    for pot in (False, True):
        d = eng.diagnostics(potential=pot)
        assert d == bh_amd.Diagnostics(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert len(eng.compute_potential()) == 0
    eng.close()


def test_multi_handle_equals_single_engine(monkeypatch):
    """Every member builds, member 0 evaluates: phi, the sums and the state that follows equal
    the one-GPU engine's, before and after steps (whose builds are LET builds)."""
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    arrs, cfg = scenes.two_disks(1500, 500), make_cfg(theta=0.5)
    one = _engine(arrs, cfg)
    two = _engine(arrs, cfg, devices=[0, 0])
    assert two.multi_world() == 2
    for rnd in range(2):
        _assert_bits(two.compute_potential(), one.compute_potential(), f"phi, round {rnd}")
        assert two.diagnostics(potential=True) == one.diagnostics(potential=True)
        assert two.diagnostics(potential=False) == one.diagnostics(potential=False)
        one.step(2)
        two.step(2)
        for name, u, v in zip(FIELDS, two.get_bodies(), one.get_bodies()):
            _assert_bits(u, v, f"{name}, round {rnd}")
    logs = [two.member(r).collective_log() for r in range(2)]
    assert np.array_equal(logs[0], logs[1])
    assert two.potential_kernel_ms() > 0.0
    two.close()
    one.close()


def test_async_guard():
    arrs = scenes.two_disks(300, 100)
    eng = _engine(arrs, make_cfg(theta=0.5))
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        for call in (eng.compute_potential, lambda: eng.diagnostics(potential=True),
                     lambda: eng.diagnostics(potential=False)):
            with pytest.raises(bh_amd.BhError) as ei:
                call()
            assert ei.value.rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    assert len(eng.compute_potential()) == eng.num_bodies()
    eng.close()


def test_potential_kernel_ms():
    eng = _engine(scenes.two_disks(1500, 500), make_cfg(theta=0.5))
    assert eng.potential_kernel_ms() == 0.0
    eng.compute_potential()
    ms = eng.potential_kernel_ms()
    assert 0.0 < ms < 1000.0
    eng.close()


def test_energy_bookkeeping():
    """merge off, theta = 0: the energy drift over 20 steps against the same quantity of the C
    oracle's (bit-identical) trajectory with the checker's energy; only the summation order
    differs.  The drift is printed."""
    arrs = scenes.two_disks(600, 200)
    cfg = make_cfg(theta=0.0, merge_min_dist=0.0)
    eng = _engine(arrs, cfg)
    d0 = eng.diagnostics(potential=True)
    eng.step(20)
    end = eng.get_bodies()
    d1 = eng.diagnostics(potential=True)
    drift = abs(d1.energy - d0.energy) / abs(d0.energy)

    phi0, st0 = theta0_phi(arrs, cfg)
    e0 = sum(energy(st0, phi0))
    ref = oracle.Oracle(*st0, theta=0.0, merge_min_dist=0.0)
    ref.step(20)
    want = ref.get_bodies()
    for name, u, v in zip(FIELDS, end, want):
        _assert_bits(u, v, name)  # the two trajectories are the same
    phi1, st1 = theta0_phi(want, cfg)
    e1 = sum(energy(st1, phi1))
    drift_ref = abs(e1 - e0) / abs(e0)
    print(f"E(0) engine {d0.energy!r} checker {e0!r}; E(20) engine {d1.energy!r} checker {e1!r}; "
          f"drift engine {drift:.17e} checker {drift_ref:.17e}")
    assert drift <= drift_ref * (1.0 + 1e-9)
    eng.close()
    ref.close()


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_nbody3d_center_of_mass(n):
    rng = np.random.default_rng(100 + n)
    pos = rng.uniform(-500.0, 500.0, (3, n)).astype(np.float32)
    m = rng.uniform(0.1, 20.0, n).astype(np.float32)
    zero = np.zeros(n, dtype=np.float32)
    sim = bh_amd.NBody3D(device=0)
    sim.set(pos[0], pos[1], pos[2], zero, zero, zero, m)
    got = sim.center_of_mass_sums()
    m64 = m.astype(np.float64)
    terms = [pos[k].astype(np.float64) * m64 for k in range(3)] + [m64]
    for g, t in zip(got, terms):
        want = math.fsum(t.tolist())
        print(f"got {g!r} want {want!r} bound {sum_bound(t):.3e}")
        assert abs(g - want) <= sum_bound(t)
    assert sim.center_of_mass_sums() == got  # deterministic
    c = sim.center_of_mass()
    assert c == (got[0] / got[3], got[1] / got[3], got[2] / got[3])
    sim.step(2)  # the sums follow the current buffer
    x, y, z, _, _, _, mm = sim.get()
    t0 = x.astype(np.float64) * mm.astype(np.float64)
    assert abs(sim.center_of_mass_sums()[0] - math.fsum(t0.tolist())) <= sum_bound(t0)
    sim.close()


def test_nbody3d_center_of_mass_of_a_massless_set():
    sim = bh_amd.NBody3D(device=0)
    z = np.zeros(300, dtype=np.float32)
    x = np.linspace(-5.0, 5.0, 300).astype(np.float32)
    sim.set(x, x, x, z, z, z, z)
    assert sim.center_of_mass() == (0.0, 0.0, 0.0)
    sim.set(*[np.zeros(0, dtype=np.float32)] * 7)
    assert sim.center_of_mass() == (0.0, 0.0, 0.0)
    sim.close()
