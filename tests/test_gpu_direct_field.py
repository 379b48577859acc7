"""GPU: bh_compute_field_direct, bh_compute_force_error, bh_direct_field_kernel_ms.

Every value check is bit-exact.  The exact field is compared with the Python checker of
tests/test_field_ref.py at theta = 0 (small shapes: one Python call per leaf per probe) and, at
larger shapes, with the engine's own theta = 0 walk -- compute_field on a second engine made with
theta = 0 from the same start arrays, a path the existing tests check against the oracle.  The
force error is compared with the C oracle's accelerations() at the engine's theta and at 0.  The
sizes come from direct_field_shape: T leaves per tile, L lanes per workgroup, NB targets per
lane, and the first target count of the second launch shape.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from test_direct_field_ref import force_error_summary
from test_field_ref import FIELDS, checker_field, make_probes, root_cell
from test_potential_ref import build, cfg_from_golden, make_cfg, params_of  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)

T, L, NB = bh_amd.direct_field_shape(1)


def _second_shape_from():
    """The first target count that launches another shape than one target does."""
    lo, hi = 1, 1 << 28
    if bh_amd.direct_field_shape(hi) == (T, L, NB):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bh_amd.direct_field_shape(mid) == (T, L, NB):
            lo = mid
        else:
            hi = mid
    return hi


BIG = _second_shape_from()
T2, L2, NB2 = bh_amd.direct_field_shape(BIG) if BIG else (T, L, NB)
assert BIG is None or BIG <= 1 << 20, "the second launch shape starts beyond what a test can run"
# a count of the second shape that leaves a partial last workgroup and a partial last wave
BIG_N = None if BIG is None else (BIG // (L2 * NB2) + 1) * (L2 * NB2) + 1


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


def _assert_state(eng, want, what=""):
    for name, a, b in zip(FIELDS, eng.get_bodies(), want):
        _assert_bits(a, b, f"{what}{name}")


def _walk(arrs, cfg, px, py, pm=None):
    """(ax, ay, phi, state after the call) of the theta = 0 walk: compute_field on an engine made
    with theta = 0 from the same arrays."""
    eng = _engine(arrs, dict(cfg, theta=0.0))
    with np.errstate(all="ignore"):
        out = eng.compute_field(px, py, pm)
    st = eng.get_bodies()
    eng.close()
    return (*out, st)


@functools.lru_cache(maxsize=None)
def _tree():
    return scenes.two_disks(1500, 500)


@functools.lru_cache(maxsize=None)
def _probes():
    return make_probes(_tree(), make_cfg(theta=0.5), 2000, 7)


@functools.lru_cache(maxsize=None)
def _walk_reference():
    """The theta = 0 walk's field of the 2000 default probes on the default tree."""
    px, py = _probes()
    return _walk(_tree(), make_cfg(theta=0.5), px, py)


@functools.lru_cache(maxsize=None)
def _small():
    return scenes.two_disks(600, 200)


@functools.lru_cache(maxsize=None)
def _small_probes():
    return make_probes(_small(), make_cfg(theta=0.5), 300, 23)


@functools.lru_cache(maxsize=None)
def _small_checker():
    px, py = _small_probes()
    return checker_field(_small(), make_cfg(theta=0.0), px, py)


# ---- the exact field -----------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted({1, 63, 64, 65, L * NB - 1, L * NB, L * NB + 1, 2000}))
def test_probe_counts(n):
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    got = eng.compute_field_direct(px[:n], py[:n])
    want = _walk_reference()
    _assert_field(got, [w[:n] for w in want[:3]])
    _assert_state(eng, want[3])
    assert 0.0 < eng.direct_field_kernel_ms() < 1000.0
    eng.close()


@pytest.mark.skipif(BIG is None, reason="one launch shape only")
def test_second_launch_shape():
    """The first count past the small shape, with a partial last workgroup and wave, in probe and
    in body mode."""
    cfg = make_cfg(theta=0.5)
    px, py = make_probes(_tree(), cfg, BIG_N, 29)
    assert bh_amd.direct_field_shape(BIG_N) == (T2, L2, NB2) != (T, L, NB)
    eng = _engine(_tree(), cfg)
    got = eng.compute_field_direct(px, py)
    want = _walk(_tree(), cfg, px, py)
    _assert_field(got, want)
    _assert_state(eng, want[3])
    eng.close()
    # body mode: every body of the small scene many times over, in a shuffled order
    n = len(_small()[0])
    idx = np.random.default_rng(31).integers(0, n, BIG_N)
    idx[:n] = np.arange(n)
    eng = _engine(_small(), cfg)
    fe = eng.force_error(idx)
    full = _oracle_pair(_small(), cfg)
    _assert_bits(fe.ax_exact, full["exact"][0][idx], "ax_exact")
    _assert_bits(fe.ay_exact, full["exact"][1][idx], "ay_exact")
    _assert_bits(fe.ax_tree, full["tree"][0][idx], "ax_tree")
    _assert_bits(fe.ay_tree, full["tree"][1][idx], "ay_tree")
    eng.close()


def _tile_cases():
    cases = [(t, 130) for t in (T - 1, T, T + 1, 2 * T + 3)]
    if BIG is not None:
        cases += [(t, BIG_N) for t in (T2 - 1, T2, T2 + 1, 2 * T2 + 3)]
    return cases


@pytest.mark.parametrize("n,n_probe", _tile_cases())
def test_leaf_tile_boundaries(n, n_probe):
    arrs = scenes.uniform(n, 1.0)
    cfg = make_cfg(theta=0.5)
    cx, cy, h = root_cell(cfg)
    assert len(arrs[0]) == n
    assert np.all((arrs[0] >= cx - h) & (arrs[0] < cx + h) & (arrs[1] >= cy - h) &
                  (arrs[1] < cy + h))  # every body is a leaf: the sequence has n records
    px, py = make_probes(arrs, cfg, 130, 37)
    if n_probe > 130:  # (the mix draws its on-body probes without replacement: uniform ones)
        rng = np.random.default_rng(39)
        px = np.concatenate([px, rng.uniform(cx - h, cx + h, n_probe - 130)])
        py = np.concatenate([py, rng.uniform(cy - h, cy + h, n_probe - 130)])
    eng = _engine(arrs, cfg)
    got = eng.compute_field_direct(px, py)
    want = _walk(arrs, cfg, px, py)
    _assert_field(got, want)
    _assert_state(eng, want[3])
    eng.close()


@pytest.mark.parametrize("theta", [0.2, 1.6])
def test_against_the_checker(theta):
    px, py = _small_probes()
    cfg = make_cfg(theta=theta)
    cx, cy, h = root_cell(cfg)
    assert np.any(np.abs(px - cx) >= h) and np.any(np.isin(px, _small()[0]))  # the mix
    eng = _engine(_small(), cfg)
    got = eng.compute_field_direct(px, py)
    want = _small_checker()
    _assert_field(got, want)
    _assert_state(eng, want[3])
    eng.close()


def test_jitter_scene():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    px, py = make_probes(arrs, cfg, 100, 13)
    eng = _engine(arrs, cfg)
    got = eng.compute_field_direct(px, py)
    want = checker_field(arrs, dict(cfg, theta=0.0), px, py)
    _assert_field(got, want)
    _assert_state(eng, want[3], "after the jitter: ")
    assert np.any(want[3][0].view(np.int64) != arrs[0].view(np.int64))  # the scene does jitter
    eng.close()


def test_massless_bodies():
    arrs = tuple(a.copy() for a in _small())
    gone = np.random.default_rng(3).choice(800, 20, replace=False)
    arrs[4][gone] = 0.0
    cfg = make_cfg(theta=0.5)
    px, py = make_probes(arrs, cfg, 190, 17)
    px = np.concatenate([px, arrs[0][gone[:10]]])  # probes on massless bodies too
    py = np.concatenate([py, arrs[1][gone[:10]]])
    eng = _engine(arrs, cfg)
    got = eng.compute_field_direct(px, py)
    want = checker_field(arrs, dict(cfg, theta=0.0), px, py)
    _assert_field(got, want)
    _assert_state(eng, want[3])
    eng.close()


def test_ieee_path_soft2_zero():
    arrs = scenes.two_disks(100, 40)
    cfg = make_cfg(theta=0.5, soft2=0.0)
    px, py = make_probes(arrs, cfg, 300, 11, on_bodies=False)
    want = checker_field(arrs, dict(cfg, theta=0.0), px, py)  # (raises on a coincidence)
    assert all(np.all(np.isfinite(w)) for w in want[:3])
    eng = _engine(arrs, cfg)
    got = eng.compute_field_direct(px, py)
    assert all(np.all(np.isfinite(g)) for g in got)
    _assert_field(got, want)
    eng.close()


def test_ieee_path_far_and_non_finite_probes():
    cfg = make_cfg(theta=0.5)
    px, py = _probes()
    fx = np.concatenate([[2.0 ** 40, -(2.0 ** 40), 300.0, 1e300, -1e200], px[:5]])
    fy = np.concatenate([[400.0, 2.0 ** 40, -(2.0 ** 45), 3.0, 1e250], py[:5]])
    eng = _engine(_tree(), cfg)
    with np.errstate(all="ignore"):
        got = eng.compute_field_direct(fx, fy)
    _assert_field(got, _walk(_tree(), cfg, fx, fy))
    # a NaN coordinate: NaN for that probe, the other 63 of its wave untouched by it
    bx, by = px[:64].copy(), py[:64].copy()
    bx[17] = math.nan
    got = eng.compute_field_direct(bx, by)
    want = _walk_reference()
    keep = np.arange(64) != 17
    for name, g, w in zip(("ax", "ay", "phi"), got, want[:3]):
        assert math.isnan(g[17]), name
        _assert_bits(g[keep], w[:64][keep], name)
    eng.close()
    # a probe on the only body at soft2 = 0
    one = (np.array([100.0]), np.array([100.0]), np.zeros(1), np.zeros(1), np.array([2.0]))
    eng = _engine(one, make_cfg(theta=0.5, soft2=0.0))
    ax, ay, phi = eng.compute_field_direct(np.array([100.0]), np.array([100.0]))
    assert math.isnan(ax[0]) and math.isnan(ay[0]) and phi[0] == -math.inf
    eng.close()


def test_probe_masses():
    px, py = _small_probes()
    px, py = px[:200], py[:200]
    cfg = make_cfg(theta=0.5)
    eng = _engine(_small(), cfg)
    unit = eng.compute_field_direct(px, py)
    _assert_field(eng.compute_field_direct(px, py, np.ones(200)), unit, "pm = 1: ")
    _assert_field(unit, [w[:200] for w in _small_checker()[:3]])
    zero = eng.compute_field_direct(px, py, np.zeros(200))
    assert np.all(np.isnan(zero[0])) and np.all(np.isnan(zero[1]))
    _assert_bits(zero[2], unit[2], "phi at pm = 0")
    pm = np.random.default_rng(9).uniform(0.5, 5000.0, 200)
    got = eng.compute_field_direct(px, py, pm)
    _assert_field(got, checker_field(_small(), make_cfg(theta=0.0), px, py, pm))
    eng.close()


def test_nullable_outputs():
    px, py = _probes()
    px, py = np.ascontiguousarray(px[:130]), np.ascontiguousarray(py[:130])
    eng = _engine(_tree(), make_cfg(theta=0.5))
    full = eng.compute_field_direct(px, py)
    _assert_field(full, [w[:130] for w in _walk_reference()[:3]])
    for skip in range(3):
        out = [np.full(130, 7.0) for _ in range(3)]
        ptrs = [None if k == skip else out[k].ctypes.data_as(_D) for k in range(3)]
        rc = eng._lib.bh_compute_field_direct(eng._h, 130, px.ctypes.data_as(_D),
                                              py.ctypes.data_as(_D), None, *ptrs)
        assert rc == bh_amd.BH_OK
        for k in range(3):
            if k != skip:
                _assert_bits(out[k], full[k], f"output {k} without output {skip}")
            else:
                assert np.all(out[k] == 7.0)
    ax, ay, phi = eng.compute_field_direct(px, py, want_phi=False)
    assert phi is None
    _assert_bits(ax, full[0], "ax")
    ax, ay, phi = eng.compute_field_direct(px, py, want_accel=False)
    assert ax is None and ay is None
    _assert_bits(phi, full[2], "phi")
    eng.close()


def test_no_probes():
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    assert eng.direct_field_kernel_ms() == 0.0
    ax, ay, phi = eng.compute_field_direct(np.zeros(0), np.zeros(0))
    assert len(ax) == len(ay) == len(phi) == 0
    assert eng.direct_field_kernel_ms() == 0.0
    _assert_state(eng, _walk_reference()[3])  # the build still happened
    eng.compute_field_direct(px[:10], py[:10])
    ms = eng.direct_field_kernel_ms()
    assert ms > 0.0
    eng.compute_field_direct(np.zeros(0), np.zeros(0))
    assert eng.direct_field_kernel_ms() == ms
    rc = eng._lib.bh_compute_field_direct(eng._h, 0, None, None, None, None, None, None)
    assert rc == bh_amd.BH_OK  # NULL px / py are fine without probes
    eng.close()


def test_empty_and_one_body_trees():
    px, py = _probes()
    px, py = px[:70], py[:70]
    cfg = make_cfg(theta=0.5)
    empty = tuple(np.zeros(0) for _ in range(5))
    eng = _engine(empty, cfg)
    ax, ay, phi = eng.compute_field_direct(px, py)
    eng.close()
    _assert_bits(ax, np.zeros(70), "ax")
    _assert_bits(ay, np.zeros(70), "ay")
    _assert_bits(phi, -np.zeros(70), "phi")  # -(G * 0.0)
    one = (np.array([700.0]), np.array([300.0]), np.zeros(1), np.zeros(1), np.array([5.0]))
    px = np.concatenate([px, [700.0]])
    py = np.concatenate([py, [300.0]])
    eng = _engine(one, cfg)
    got = eng.compute_field_direct(px, py)
    eng.close()
    _assert_field(got, checker_field(one, dict(cfg, theta=0.0), px, py))
    assert got[2][-1] == -80.0 * 5.0 and got[0][-1] == 0.0 and got[1][-1] == 0.0
    # a body outside the root cell is not in the tree: nobody feels it
    out = (np.array([1e6]), np.array([300.0]), np.zeros(1), np.zeros(1), np.array([5.0]))
    eng = _engine(out, cfg)
    ax, ay, phi = eng.compute_field_direct(px, py)
    eng.close()
    _assert_bits(ax, np.zeros(71), "ax")
    _assert_bits(phi, -np.zeros(71), "phi")


def test_invalid_arguments():
    eng = _engine(scenes.two_disks(100, 40), make_cfg(theta=0.5))
    p = np.zeros(4)
    dp = p.ctypes.data_as(_D)
    lib = eng._lib
    for n, x, y in ((-1, dp, dp), ((1 << 28) + 1, dp, dp), (4, None, dp), (4, dp, None)):
        assert lib.bh_compute_field_direct(eng._h, n, x, y, None, None, None,
                                           None) == bh_amd.BH_E_INVALID
        assert b"bh_compute_field_direct" in lib.bh_last_error(eng._h)
    assert lib.bh_direct_field_kernel_ms(eng._h, None) == bh_amd.BH_E_INVALID
    eng.close()


def test_async_guard():
    arrs = scenes.two_disks(300, 100)
    eng = _engine(arrs, make_cfg(theta=0.5))
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        with pytest.raises(bh_amd.BhError) as ei:
            eng.compute_field_direct(np.array([1.0]), np.array([2.0]))
        assert ei.value.rc == bh_amd.BH_E_STATE
        with pytest.raises(bh_amd.BhError) as ei:
            eng.force_error(np.array([0]))
        assert ei.value.rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    assert len(eng.compute_field_direct(np.array([1.0]), np.array([2.0]))[2]) == 1
    assert eng.force_error(np.array([0])).n_sample == 1
    eng.close()


def test_repeatable():
    px, py = _probes()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    first = eng.compute_field_direct(px, py)
    second = eng.compute_field_direct(px, py)
    _assert_field(second, first)
    # fewer probes after more (the buffers are larger than the call)
    _assert_field(eng.compute_field_direct(px[:100], py[:100]), [f[:100] for f in first])
    eng.close()


def test_multi_handle_equals_single_engine(monkeypatch):
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    px, py = _probes()
    px, py = px[:300], py[:300]
    cfg = make_cfg(theta=0.5)
    idx = np.random.default_rng(41).choice(2000, 200, replace=False)
    one = _engine(_tree(), cfg)
    two = _engine(_tree(), cfg, devices=[0, 0])
    assert two.multi_world() == 2
    for rnd in range(2):
        _assert_field(two.compute_field_direct(px, py), one.compute_field_direct(px, py),
                      f"round {rnd}: ")
        if rnd == 0:
            _assert_field(two.compute_field_direct(px, py),
                          [w[:300] for w in _walk_reference()[:3]])
        a, b = two.force_error(idx), one.force_error(idx)
        for f in ("ax_tree", "ay_tree", "ax_exact", "ay_exact", "max_rel", "mean_rel", "rms_rel"):
            _assert_bits(getattr(a, f), getattr(b, f), f"{f}, round {rnd}")
        assert (a.n_used, a.worst) == (b.n_used, b.worst) and a.n_used == 200
        one.step(2)
        two.step(2)
        _assert_state(two, one.get_bodies(), f"round {rnd}: ")
    logs = [two.member(r).collective_log() for r in range(2)]
    assert np.array_equal(logs[0], logs[1])
    assert two.direct_field_kernel_ms() > 0.0
    two.close()
    one.close()


def test_after_stepping():
    """After step(3) merges have shrunk N, the tree is the carried one and the lane map is live.
    The walk engine is stepped alike at the same theta and set to theta = 0 for its query."""
    arrs = scenes.config_scene("c1_baseline")
    cfg = make_cfg(theta=0.5)
    eng, walk = _engine(arrs, cfg), _engine(arrs, cfg)
    eng.step(3)
    walk.step(3)
    now = eng.get_bodies()
    assert len(now[0]) < len(arrs[0])
    px, py = make_probes(now, cfg, 200, 19)
    got = eng.compute_field_direct(px, py)
    walk.set_params(params_of(dict(cfg, theta=0.0)))
    want = walk.compute_field(px, py)
    _assert_field(got, want, "after step(3): ")
    _assert_state(eng, walk.get_bodies(), "after step(3): ")
    eng.close()
    walk.close()


# ---- the force error -----------------------------------------------------------------------

def _oracle_accel(arrs, cfg):
    ref = oracle.Oracle(*arrs, p=oracle.params(**cfg))
    ax, ay = ref.accelerations()
    st = ref.get_bodies()
    ref.close()
    return ax, ay, st


@functools.lru_cache(maxsize=None)
def _oracle_pair_cached(key):
    arrs, cfg = _PAIR_ARGS[key]
    ax, ay, st = _oracle_accel(arrs, cfg)
    ex, ey, st0 = _oracle_accel(arrs, dict(cfg, theta=0.0))
    for a, b in zip(st, st0):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))  # the build knows no theta
    return dict(tree=(ax, ay), exact=(ex, ey), state=st)


_PAIR_ARGS = {}


def _oracle_pair(arrs, cfg):
    """The C oracle's accelerations() at cfg's theta and at theta = 0 and the state after."""
    key = (id(arrs), tuple(sorted(cfg.items())))
    _PAIR_ARGS[key] = (arrs, cfg)
    return _oracle_pair_cached(key)


def _assert_force_error(fe, want, idx, what=""):
    _assert_bits(fe.ax_tree, want["tree"][0][idx], what + "ax_tree")
    _assert_bits(fe.ay_tree, want["tree"][1][idx], what + "ay_tree")
    _assert_bits(fe.ax_exact, want["exact"][0][idx], what + "ax_exact")
    _assert_bits(fe.ay_exact, want["exact"][1][idx], what + "ay_exact")


def _assert_summary(fe):
    s = force_error_summary(fe.ax_tree, fe.ay_tree, fe.ax_exact, fe.ay_exact)
    assert (fe.n_sample, fe.n_used, fe.worst) == (s["n_sample"], s["n_used"], s["worst"])
    for f in ("max_rel", "mean_rel", "rms_rel"):
        _assert_bits(getattr(fe, f), s[f], f)
    return s


@pytest.mark.parametrize("theta", [0.2, 0.5, 1.0])
def test_force_error_against_the_oracle(theta):
    arrs, cfg = _small(), make_cfg(theta=theta)
    n = len(arrs[0])
    idx = np.arange(n)
    want = _oracle_pair(arrs, cfg)
    four = (*want["tree"], *want["exact"])
    assert all(np.all(np.isfinite(a)) for a in four)  # n_used == n_sample: the test's condition
    assert np.all(np.hypot(*want["exact"]) > 0.0)
    eng = _engine(arrs, cfg)
    fe = eng.force_error(idx)
    _assert_force_error(fe, want, idx)
    _assert_state(eng, want["state"])
    s = _assert_summary(fe)
    assert s["n_used"] == fe.n_sample == n
    if theta == 0.5:
        assert 0.0 < fe.max_rel < 1.0
    assert 0.0 < eng.direct_field_kernel_ms() < 1000.0
    eng.close()


def test_force_error_at_theta_zero():
    arrs, cfg = _small(), make_cfg(theta=0.0)
    eng = _engine(arrs, cfg)
    fe = eng.force_error(np.arange(len(arrs[0])))
    _assert_bits(fe.ax_tree, fe.ax_exact, "ax")
    _assert_bits(fe.ay_tree, fe.ay_exact, "ay")
    assert fe.max_rel == fe.mean_rel == fe.rms_rel == 0.0 and fe.worst == 0
    assert fe.n_used == fe.n_sample
    eng.close()


@pytest.mark.parametrize("n", [T - 1, T + 1, 2 * T + 3])
def test_force_error_leaf_tile_boundaries(n):
    arrs = scenes.uniform(n, 1.0)
    cfg = make_cfg(theta=0.5)
    eng, exact = _engine(arrs, cfg), _engine(arrs, dict(cfg, theta=0.0))
    fe = eng.force_error(np.arange(n))
    ex, ey = exact.compute_accelerations()
    _assert_bits(fe.ax_exact, ex, "ax_exact")
    _assert_bits(fe.ay_exact, ey, "ay_exact")
    _assert_state(eng, exact.get_bodies())
    eng.close()
    exact.close()


def test_force_error_idx_handling():
    arrs, cfg = _small(), make_cfg(theta=0.5)
    n = len(arrs[0])
    want = _oracle_pair(arrs, cfg)
    eng = _engine(arrs, cfg)
    lib = eng._lib
    # a failed call launches nothing: the state is the uploaded list
    for bad in (n, -1):
        idx = np.array([3, bad, 5], dtype=np.int64)
        rc = lib.bh_compute_force_error(eng._h, 3, idx.ctypes.data_as(_I64P), None, None, None,
                                        None, None)
        assert rc == bh_amd.BH_E_INVALID
        assert b"bh_compute_force_error" in lib.bh_last_error(eng._h)
    for k in (-1, (1 << 28) + 1):
        idx = np.zeros(1, dtype=np.int64)
        assert lib.bh_compute_force_error(eng._h, k, idx.ctypes.data_as(_I64P), None, None, None,
                                          None, None) == bh_amd.BH_E_INVALID
    assert lib.bh_compute_force_error(eng._h, 2, None, None, None, None, None,
                                      None) == bh_amd.BH_E_INVALID
    _assert_state(eng, arrs, "after refused calls: ")
    assert eng.direct_field_kernel_ms() == 0.0
    # no samples: the build and the evaluation, no all-pairs kernel, zeros and worst = -1
    fe = eng.force_error(np.zeros(0, dtype=np.int64))
    assert (fe.n_sample, fe.n_used, fe.worst) == (0, 0, -1)
    assert fe.max_rel == fe.mean_rel == fe.rms_rel == 0.0
    assert eng.direct_field_kernel_ms() == 0.0
    _assert_state(eng, want["state"])
    # 65 entries, unsorted, with duplicates
    idx = np.random.default_rng(43).integers(0, n, 65)
    idx[7] = idx[40] = idx[64]
    fe = eng.force_error(idx)
    _assert_force_error(fe, want, idx)
    _assert_summary(fe)
    # each nullable output skipped in turn
    i64 = np.ascontiguousarray(idx, dtype=np.int64)
    full = (fe.ax_tree, fe.ay_tree, fe.ax_exact, fe.ay_exact)
    for skip in range(5):
        out = [np.full(65, 7.0) for _ in range(4)]
        ptrs = [None if k == skip else out[k].ctypes.data_as(_D) for k in range(4)]
        s = bh_amd.BhForceError()
        rc = lib.bh_compute_force_error(eng._h, 65, i64.ctypes.data_as(_I64P), *ptrs,
                                        None if skip == 4 else ctypes.byref(s))
        assert rc == bh_amd.BH_OK
        for k in range(4):
            if k != skip:
                _assert_bits(out[k], full[k], f"output {k} without output {skip}")
        if skip != 4:
            assert (s.n_sample, s.n_used, s.worst) == (65, fe.n_used, fe.worst)
            _assert_bits(s.max_rel, fe.max_rel, "max_rel")
    eng.close()


def test_force_error_outside_bodies():
    z = np.load(os.path.join(GOLDEN, "outside_153.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    cx, cy, h = root_cell(cfg)
    outside = np.flatnonzero((np.abs(arrs[0] - cx) >= h) | (np.abs(arrs[1] - cy) >= h))
    assert outside.size > 0
    want = _oracle_pair(arrs, cfg)
    eng = _engine(arrs, cfg)
    fe = eng.force_error(outside)
    _assert_force_error(fe, want, outside)
    fe = eng.force_error(np.arange(len(arrs[0])))
    _assert_force_error(fe, want, np.arange(len(arrs[0])), "every body: ")
    eng.close()


def test_force_error_massless_bodies():
    arrs = tuple(a.copy() for a in _small())
    n = len(arrs[0])
    gone = np.array([17, 640])
    arrs[4][gone] = 0.0
    cfg = make_cfg(theta=0.5)
    want = _oracle_pair(arrs, cfg)
    idx = np.arange(n)
    eng = _engine(arrs, cfg)
    fe = eng.force_error(idx)
    for a in (fe.ax_tree, fe.ay_tree, fe.ax_exact, fe.ay_exact):
        assert np.all(np.isnan(a[gone]))
    rest = np.setdiff1d(idx, gone)
    for got, ref in zip((fe.ax_tree, fe.ay_tree, fe.ax_exact, fe.ay_exact),
                        (*want["tree"], *want["exact"])):
        _assert_bits(got[rest], ref[rest], "the rest")
    assert fe.n_used == fe.n_sample - 2
    _assert_summary(fe)
    eng.close()


def test_force_error_ieee_path():
    """soft2 = 0: the wave sums on the IEEE path, where the own leaf is skipped by branch."""
    arrs = scenes.two_disks(100, 40)
    cfg = make_cfg(theta=0.5, soft2=0.0)
    want = _oracle_pair(arrs, cfg)
    assert all(np.all(np.isfinite(a)) for a in want["exact"])
    idx = np.arange(len(arrs[0]))
    eng = _engine(arrs, cfg)
    fe = eng.force_error(idx)
    _assert_force_error(fe, want, idx)
    eng.close()


def test_force_error_state_semantics():
    cfg = make_cfg(theta=0.5)
    a, b = _engine(_tree(), cfg), _engine(_tree(), cfg)
    a.force_error(sample=500)
    b.compute_accelerations()
    a.step(5)
    b.step(5)
    _assert_state(a, b.get_bodies())
    a.close()
    b.close()


def test_force_error_after_stepping():
    arrs = scenes.config_scene("c1_baseline")
    cfg = make_cfg(theta=0.5)
    eng = _engine(arrs, cfg)
    eng.step(3)
    now = eng.get_bodies()
    n = len(now[0])
    assert n < len(arrs[0])
    idx = np.random.default_rng(47).choice(n, 300, replace=False)
    fe = eng.force_error(idx)
    want = _oracle_pair(now, cfg)
    _assert_force_error(fe, want, idx, "after step(3): ")
    _assert_state(eng, want["state"], "after step(3): ")
    _assert_summary(fe)
    eng.close()


def test_force_error_default_sample():
    arrs, cfg = _small(), make_cfg(theta=0.5)
    n = len(arrs[0])
    eng = _engine(arrs, cfg)
    fe = eng.force_error(sample=100, seed=3)
    want_idx = np.sort(np.random.default_rng(3).choice(n, 100, replace=False))
    assert np.array_equal(fe.idx, want_idx) and fe.n_sample == 100
    _assert_force_error(fe, _oracle_pair(arrs, cfg), want_idx)
    fe = eng.force_error(sample=10 ** 6)  # more than N: every body once
    assert np.array_equal(fe.idx, np.arange(n))
    eng.close()
