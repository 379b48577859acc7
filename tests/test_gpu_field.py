"""GPU: bh_compute_field / bh_field_kernel_ms.

Every value check is bit-exact against the Python checker of tests/test_field_ref.py built from
the same start state: the probe is a fresh body that is not in the tree, walked by the oracle's
own accumulate_force (force) and by the potential checker's walk (phi).  The reference of the
default tree is computed once and shared.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from test_field_ref import FIELDS, checker_field, make_probes
from test_potential_ref import build, cfg_from_golden, make_cfg, params_of, potential_walk

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)


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


def _assert_field(got, want, what=""):
    for name, g, w in zip(("ax", "ay", "phi"), got, want[:3]):
        _assert_bits(g, w, f"{what}{name}")


def _check(arrs, cfg, px, py, pm=None, state=True):
    """Engine field and the state after the call against the checker's, bit for bit."""
    eng = _engine(arrs, cfg)
    got = eng.compute_field(px, py, pm)
    want = checker_field(arrs, cfg, px, py, pm)
    _assert_field(got, want)
    if state:
        for name, a, b in zip(FIELDS, eng.get_bodies(), want[3]):
            _assert_bits(a, b, name)  # the build's jitter is part of the call
    eng.close()
    return got


@functools.lru_cache(maxsize=None)
def _tree():
    return scenes.two_disks(1500, 500)


@functools.lru_cache(maxsize=None)
def _probes():
    return make_probes(_tree(), make_cfg(theta=0.5), 2000, 7)


@functools.lru_cache(maxsize=None)
def _reference(theta, n):
    """The checker's (ax, ay, phi, state) for the first n default probes on the default tree."""
    px, py = _probes()
    return checker_field(_tree(), make_cfg(theta=theta), px[:n], py[:n])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 2000])
def test_probe_counts(n):
    """Wave and workgroup boundaries of the launch; the mix has probes outside the root cell and
    probes exactly on bodies at every count from 63 up."""
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    got = eng.compute_field(px[:n], py[:n])
    want = _reference(0.5, 2000)
    _assert_field(got, [w[:n] for w in want[:3]])
    for name, a, b in zip(FIELDS, eng.get_bodies(), want[3]):
        _assert_bits(a, b, name)
    assert 0.0 < eng.field_kernel_ms() < 1000.0
    eng.close()


def test_no_probes():
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    assert eng.field_kernel_ms() == 0.0
    ax, ay, phi = eng.compute_field(np.zeros(0), np.zeros(0))
    assert len(ax) == len(ay) == len(phi) == 0
    assert eng.field_kernel_ms() == 0.0
    # the build still happened: the state is the one compute_accelerations leaves
    for name, a, b in zip(FIELDS, eng.get_bodies(), _reference(0.5, 2000)[3]):
        _assert_bits(a, b, name)
    eng.compute_field(px[:10], py[:10])
    ms = eng.field_kernel_ms()
    assert ms > 0.0
    eng.compute_field(np.zeros(0), np.zeros(0))
    assert eng.field_kernel_ms() == ms
    # NULL px / py are fine without probes
    rc = eng._lib.bh_compute_field(eng._h, 0, None, None, None, None, None, None)
    assert rc == bh_amd.BH_OK
    eng.close()


@pytest.mark.parametrize("theta", [0.2, 0.5, 1.0, 1.6])
def test_theta_sweep(theta):
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=theta))
    got = eng.compute_field(px[:300], py[:300])
    _assert_field(got, _reference(theta, 300))
    eng.close()


def test_theta0_opens_everything():
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.0))
    got = eng.compute_field(px[:130], py[:130])
    _assert_field(got, _reference(0.0, 130))
    eng.close()


def test_slot_collision_on_the_ieee_path():
    """soft2 = 0 walks the IEEE path, the one that compares leaf slots in the force walk; with
    more probes than bodies, probe i coexists with body slot i and must still feel it.  No probe
    coincides with a body or a centre of mass: the checker raises nothing (it would divide by
    zero) and every output is finite."""
    arrs = scenes.two_disks(100, 40)
    cfg = make_cfg(theta=0.5, soft2=0.0)
    px, py = make_probes(arrs, cfg, 300, 11, on_bodies=False)
    want = checker_field(arrs, cfg, px, py)  # (raises on a coincidence)
    assert all(np.all(np.isfinite(w)) for w in want[:3])
    eng = _engine(arrs, cfg)
    got = eng.compute_field(px, py)
    assert all(np.all(np.isfinite(g)) for g in got)
    _assert_field(got, want)
    eng.close()


def test_coincident_probes_on_the_fast_path():
    """65 probes exactly on 65 bodies at soft2 = 1: phi carries the body's own m / sqrt(soft2)
    that the body's potential leaves out, the force gains an exact zero.  (A body whose walk
    accepts a cell around itself -- a cell of side < theta * sqrt(soft2) always is -- never
    reaches its own leaf: probe and body then see the same nodes.)"""
    arrs = _tree()
    cfg = make_cfg(theta=0.5, soft2=1.0)
    on = np.random.default_rng(5).choice(len(arrs[0]), 65, replace=False)
    px, py, pm = arrs[0][on].copy(), arrs[1][on].copy(), arrs[4][on].copy()
    ax, ay, phi = _check(arrs, cfg, px, py, pm)
    assert np.all(np.isfinite(ax)) and np.all(np.isfinite(ay))
    pe, root = build(arrs, cfg)
    gained = 0
    for j, i in enumerate(on):
        assert pe.bodies[i].x == px[j] and pe.bodies[i].y == py[j]  # (not jittered)
        own = potential_walk(root, pe.bodies[i], cfg)
        if phi[j] == own:
            continue
        assert phi[j] < own
        assert math.isclose(own - phi[j], cfg["G"] * pm[j], rel_tol=1e-9)
        gained += 1
    assert gained > 0


def test_ieee_known_answers():
    one = (np.array([100.0]), np.array([100.0]), np.zeros(1), np.zeros(1), np.array([2.0]))
    eng = _engine(one, make_cfg(theta=0.5, soft2=0.0))
    ax, ay, phi = eng.compute_field(np.array([100.0]), np.array([100.0]))
    assert math.isnan(ax[0]) and math.isnan(ay[0]) and phi[0] == -math.inf
    eng.close()
    # far outside the fast path's position bound: the wave walks the IEEE path
    cfg = make_cfg(theta=0.5)
    px, py = _probes()
    fx = np.concatenate([[2.0 ** 40, -(2.0 ** 40), 300.0, 1e300, -1e200], px[:5]])
    fy = np.concatenate([[400.0, 2.0 ** 40, -(2.0 ** 45), 3.0, 1e250], py[:5]])
    with np.errstate(over="ignore"):
        _check(_tree(), cfg, fx, fy, state=False)
    # a NaN coordinate: NaN for that probe, the other 63 of its wave untouched by it
    bx, by = px[:64].copy(), py[:64].copy()
    bx[17] = math.nan
    eng = _engine(_tree(), cfg)
    got = eng.compute_field(bx, by)
    want = _reference(0.5, 2000)
    keep = np.arange(64) != 17
    for name, g, w in zip(("ax", "ay", "phi"), got, want[:3]):
        assert math.isnan(g[17]), name
        _assert_bits(g[keep], w[:64][keep], name)
    # infinite coordinates are walked too
    got = eng.compute_field(np.array([math.inf, 5.0]), np.array([5.0, -math.inf]))
    assert all(len(g) == 2 for g in got)
    eng.close()


def test_probe_masses():
    px, py = _probes()
    px, py = px[:200], py[:200]
    cfg = make_cfg(theta=0.5)
    eng = _engine(_tree(), cfg)
    unit = eng.compute_field(px, py)
    _assert_field(eng.compute_field(px, py, np.ones(200)), unit, "pm = 1: ")
    _assert_field(unit, [w[:200] for w in _reference(0.5, 2000)[:3]])
    zero = eng.compute_field(px, py, np.zeros(200))
    assert np.all(np.isnan(zero[0])) and np.all(np.isnan(zero[1]))
    _assert_bits(zero[2], unit[2], "phi at pm = 0")
    eng.close()
    pm = np.random.default_rng(9).uniform(0.5, 5000.0, 200)
    _check(_tree(), cfg, px, py, pm, state=False)


def test_empty_and_one_body_trees():
    px, py = _probes()
    px, py = px[:70], py[:70]
    empty = tuple(np.zeros(0) for _ in range(5))
    ax, ay, phi = _check(empty, make_cfg(theta=0.5), px, py)
    _assert_bits(ax, np.zeros(70), "ax")
    _assert_bits(ay, np.zeros(70), "ay")
    _assert_bits(phi, -np.zeros(70), "phi")  # -(G * 0.0)
    one = (np.array([700.0]), np.array([300.0]), np.zeros(1), np.zeros(1), np.array([5.0]))
    px = np.concatenate([px, [700.0]])
    py = np.concatenate([py, [300.0]])
    ax, ay, phi = _check(one, make_cfg(theta=0.5), px, py)
    assert phi[-1] == -80.0 * 5.0 and ax[-1] == 0.0 and ay[-1] == 0.0
    # a body outside the root cell is not in the tree: nobody feels it
    out = (np.array([1e6]), np.array([300.0]), np.zeros(1), np.zeros(1), np.array([5.0]))
    ax, ay, phi = _check(out, make_cfg(theta=0.5), px, py)
    _assert_bits(phi, -np.zeros(71), "phi")


def test_jitter_scene():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    px, py = make_probes(arrs, cfg, 100, 13)
    eng = _engine(arrs, cfg)
    got = eng.compute_field(px, py)
    want = checker_field(arrs, cfg, px, py)
    _assert_field(got, want)
    state = eng.get_bodies()
    _assert_bits(state[0], want[3][0], "x after the jitter")
    _assert_bits(state[1], want[3][1], "y after the jitter")
    assert np.any(state[0].view(np.int64) != arrs[0].view(np.int64))  # the scene does jitter
    eng.close()


def test_massless_bodies():
    arrs = tuple(a.copy() for a in scenes.two_disks(600, 200))
    gone = np.random.default_rng(3).choice(800, 20, replace=False)
    arrs[4][gone] = 0.0
    cfg = make_cfg(theta=0.5)
    px, py = make_probes(arrs, cfg, 190, 17)
    px = np.concatenate([px, arrs[0][gone[:10]]])  # probes on massless bodies too
    py = np.concatenate([py, arrs[1][gone[:10]]])
    _check(arrs, cfg, px, py)


def test_state_semantics_of_compute_accelerations():
    px, py = _probes()
    cfg = make_cfg(theta=0.5)
    a, b = _engine(_tree(), cfg), _engine(_tree(), cfg)
    a.compute_field(px[:500], py[:500])
    b.compute_accelerations()
    a.step(5)
    b.step(5)
    for name, u, v in zip(FIELDS, a.get_bodies(), b.get_bodies()):
        _assert_bits(u, v, name)
    a.close()
    b.close()


def test_after_stepping():
    """After step(3) merges have shrunk N, the tree is the carried one and the lane map is live."""
    arrs = scenes.config_scene("c1_baseline")
    cfg = make_cfg(theta=0.5)
    eng = _engine(arrs, cfg)
    eng.step(3)
    now = eng.get_bodies()
    px, py = make_probes(now, cfg, 200, 19)
    got = eng.compute_field(px, py)
    want = checker_field(now, cfg, px, py)
    _assert_field(got, want, "after step(3): ")
    for name, a, b in zip(FIELDS, eng.get_bodies(), want[3]):
        _assert_bits(a, b, name)
    eng.close()


def test_repeatable():
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    first = eng.compute_field(px, py)
    second = eng.compute_field(px, py)
    _assert_field(second, first)
    # fewer probes after more (the buffers are larger than the call), then more again
    _assert_field(eng.compute_field(px[:100], py[:100]), [f[:100] for f in first])
    eng.close()


def test_nullable_outputs():
    px, py = _probes()
    px, py = np.ascontiguousarray(px[:130]), np.ascontiguousarray(py[:130])
    eng = _engine(_tree(), make_cfg(theta=0.5))
    full = eng.compute_field(px, py)
    for skip in range(3):
        out = [np.full(130, 7.0) for _ in range(3)]
        ptrs = [None if k == skip else out[k].ctypes.data_as(_D) for k in range(3)]
        rc = eng._lib.bh_compute_field(eng._h, 130, px.ctypes.data_as(_D), py.ctypes.data_as(_D),
                                       None, *ptrs)
        assert rc == bh_amd.BH_OK
        for k in range(3):
            if k != skip:
                _assert_bits(out[k], full[k], f"output {k} without output {skip}")
    ax, ay, phi = eng.compute_field(px, py, want_phi=False)
    assert phi is None
    _assert_bits(ax, full[0], "ax")
    ax, ay, phi = eng.compute_field(px, py, want_accel=False)
    assert ax is None and ay is None
    _assert_bits(phi, full[2], "phi")
    eng.close()


def test_invalid_arguments():
    eng = _engine(scenes.two_disks(100, 40), make_cfg(theta=0.5))
    p = np.zeros(4)
    dp = p.ctypes.data_as(_D)
    lib = eng._lib
    assert lib.bh_compute_field(None, 4, dp, dp, None, None, None, None) == bh_amd.BH_E_INVALID
    for n, x, y in ((-1, dp, dp), ((1 << 28) + 1, dp, dp), (4, None, dp), (4, dp, None)):
        assert lib.bh_compute_field(eng._h, n, x, y, None, None, None, None) == bh_amd.BH_E_INVALID
        assert b"bh_compute_field" in lib.bh_last_error(eng._h)
    ms = ctypes.c_double(1.0)
    assert lib.bh_field_kernel_ms(None, ctypes.byref(ms)) == bh_amd.BH_E_INVALID
    assert lib.bh_field_kernel_ms(eng._h, None) == bh_amd.BH_E_INVALID
    eng.close()


def test_async_guard():
    arrs = scenes.two_disks(300, 100)
    eng = _engine(arrs, make_cfg(theta=0.5))
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        with pytest.raises(bh_amd.BhError) as ei:
            eng.compute_field(np.array([1.0]), np.array([2.0]))
        assert ei.value.rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    assert len(eng.compute_field(np.array([1.0]), np.array([2.0]))[2]) == 1
    eng.close()


def test_multi_handle_equals_single_engine(monkeypatch):
    """Every member builds, member 0 evaluates and answers: the field and the state that follows
    equal the one-GPU engine's, before and after steps."""
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    px, py = _probes()
    px, py = px[:300], py[:300]
    cfg = make_cfg(theta=0.5)
    one = _engine(_tree(), cfg)
    two = _engine(_tree(), cfg, devices=[0, 0])
    assert two.multi_world() == 2
    for rnd in range(2):
        _assert_field(two.compute_field(px, py), one.compute_field(px, py), f"round {rnd}: ")
        if rnd == 0:
            _assert_field(two.compute_field(px, py), _reference(0.5, 300))
        one.step(2)
        two.step(2)
        for name, u, v in zip(FIELDS, two.get_bodies(), one.get_bodies()):
            _assert_bits(u, v, f"{name}, round {rnd}")
    logs = [two.member(r).collective_log() for r in range(2)]
    assert np.array_equal(logs[0], logs[1])
    assert two.field_kernel_ms() > 0.0
    two.close()
    one.close()
