"""GPU: bh_compute_field_grid / bh_field_grid_kernel_ms.

Every value check is bit-exact: against the Python checker of tests/test_field_ref.py on the
host-made coordinates of the grid (tests/test_field_grid_ref.py grid_coords: one multiply and one
add), or against Engine.compute_field on a twin engine holding the same state.  x0 and dx are
non-dyadic, so that a fused multiply-add in the kernel's coordinates would change bits.  The
checker's reference of the default tree is computed once, over all the small grids, and shared.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from test_field_grid_ref import grid_coords, shape_boundaries, stats_dict, stats_rule
from test_field_ref import FIELDS, checker_field
from test_potential_ref import cfg_from_golden, make_cfg, params_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)

# the default grid geometry: a 64 x 33 grid of it spans the 2400 x 800 world
X0, Y0, DX, DY = 3.1, 3.3, 37.7, 24.3
SMALL = [(1, 1), (64, 1), (1, 65), (8, 8), (9, 9), (13, 7), (64, 33)]


def _engine(arrs, cfg, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    return eng


def _assert_bits(got, want, what):
    got = np.asarray(got, dtype=np.float64).ravel()
    want = np.asarray(want, dtype=np.float64).ravel()
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


def _assert_stats(s, planes, what=""):
    """The device's stats against the NumPy rule on the planes: values by ==, the rest exact."""
    got, want = stats_dict(s), stats_rule(*planes)
    assert got == want, f"{what}{got} vs {want}"  # (== on floats: zeros compare by value)


@functools.lru_cache(maxsize=None)
def _tree():
    return scenes.two_disks(1500, 500)


@functools.lru_cache(maxsize=None)
def _reference():
    """The checker's field on the default tree (theta 0.5) at the points of every SMALL grid, one
    call: {(nx, ny): (ax, ay, phi)} and the state after the build."""
    pts = [grid_coords(X0, Y0, DX, DY, nx, ny) for nx, ny in SMALL]
    px = np.concatenate([p[0] for p in pts])
    py = np.concatenate([p[1] for p in pts])
    ax, ay, phi, st = checker_field(_tree(), make_cfg(theta=0.5), px, py)
    out, lo = {}, 0
    for nx, ny in SMALL:
        hi = lo + nx * ny
        out[(nx, ny)] = (ax[lo:hi], ay[lo:hi], phi[lo:hi])
        lo = hi
    return out, st


def _check(arrs, cfg, grid, state=True):
    """Engine grid field and the state after the call against the checker's, bit for bit."""
    eng = _engine(arrs, cfg)
    got = eng.compute_field_grid(*grid)
    with np.errstate(all="ignore"):
        want = checker_field(arrs, cfg, *grid_coords(*grid))
    assert got[0].shape == got[1].shape == got[2].shape == (grid[5], grid[4])
    _assert_field(got, want)
    if state:
        _assert_state(eng, want[3])  # the build's jitter is part of the call
    eng.close()
    return got


class _Twins:
    """Two engines with the same start state: `a` answers compute_field_grid, `b` compute_field
    on the grid's host-made coordinates.  Both calls build, so the pair stays in step."""

    def __init__(self, arrs, cfg):
        self.a, self.b = _engine(arrs, cfg), _engine(arrs, cfg)

    def check(self, grid, what="", **kw):
        got = self.a.compute_field_grid(*grid, **kw)
        want = self.b.compute_field(*grid_coords(*grid))
        _assert_field(got[:3], want, what)
        return got

    def close(self):
        _assert_state(self.a, self.b.get_bodies(), "twin state: ")
        self.a.close()
        self.b.close()


# ---- values ----------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SMALL)
def test_small_grids_against_the_checker(nx, ny):
    """One lane, one row, one column, a full tile, every edge tile kind, about 2 000 points."""
    ref, state = _reference()
    eng = _engine(_tree(), make_cfg(theta=0.5))
    got = eng.compute_field_grid(X0, Y0, DX, DY, nx, ny)
    assert all(g.shape == (ny, nx) for g in got)
    _assert_field(got, ref[(nx, ny)])
    _assert_state(eng, state)
    eng.close()


def test_shape_boundaries_against_compute_field():
    """160 x 96, and one grid on each side of every boundary bh_field_grid_shape reports below
    1 << 16 points (341 columns: the rows where the tile or the workgroup changes)."""
    firsts = shape_boundaries(341, list(range(1, 194)))
    assert len(firsts) == 6 and 341 * (firsts[-1] - 1) < 1 << 16
    t = _Twins(_tree(), make_cfg(theta=0.5))
    t.check((X0, Y0, 15.1, 8.3, 160, 96), "160 x 96: ")
    for ny in firsts:
        for rows in (ny - 1, ny):
            shape = bh_amd.field_grid_shape(341, rows)
            t.check((X0, Y0, 7.03, 799.0 / rows, 341, rows), f"341 x {rows} {shape}: ")
    t.close()


def test_workgroup_boundary_against_compute_field():
    """The one boundary above 1 << 16 points: 8192 tiles, where a workgroup goes from 8 waves to
    4 (and the XCD runs from 8 workgroups to 16)."""
    assert shape_boundaries(1024, [504, 505]) == [505]
    assert [bh_amd.field_grid_shape(1024, ny)[2] for ny in (504, 505)] == [8, 4]
    t = _Twins(_tree(), make_cfg(theta=0.5))
    for ny in (504, 505):
        t.check((X0, Y0, 2.33, 1.57, 1024, ny), f"1024 x {ny}: ")
    t.close()


@pytest.mark.parametrize("theta", [0.0, 0.2, 1.0, 1.6])
def test_theta_sweep(theta):
    arrs = scenes.two_disks(150, 50) if theta == 0.0 else _tree()
    _check(arrs, make_cfg(theta=theta), (X0, Y0, 123.7, 81.3, 20, 10), state=False)


def test_grid_positions():
    t = _Twins(_tree(), make_cfg(theta=0.5))
    with np.errstate(all="ignore"):
        t.check((3000.1, -900.3, 0.7, 0.3, 20, 10), "outside the root cell: ")
        t.check((-300.1, -200.3, 150.7, 70.3, 20, 17), "straddling the root cell: ")
        t.check((2.0 ** 40, Y0, 0.7, DY, 20, 10), "x0 = 2^40: ")
        t.check((1e300, Y0, 0.7, DY, 20, 10), "x0 = 1e300: ")
        # the right column at 2^40 through a huge dx: 32 one-lane waves, every other one off the
        # fast path, in one launch
        assert bh_amd.field_grid_shape(2, 16)[:2] == (1, 1)
        far = t.check((X0, Y0, 2.0 ** 40, DY, 2, 16), "right half at 2^40: ")
        assert np.all(np.isfinite(far[2])) and np.all(far[2][:, 0] < far[2][:, 1])
        # full 8 x 8 tiles: the left tile column inside the fast path's 2^32 bound, the right
        # one beyond it
        assert bh_amd.field_grid_shape(16, 4100)[:2] == (8, 8)
        far = t.check((X0, Y0, 2.0 ** 29 + 0.7, 0.19, 16, 4100), "right tiles past 2^32: ")
        assert np.all(np.isfinite(far[2]))
        same = t.check((700.1, Y0, 0.0, DY, 20, 10), "dx = 0: ")
        for g in same:
            _assert_bits(g, np.repeat(g[:, :1], 20, axis=1), "dx = 0, every column")
        down = t.check((X0, 780.3, DX, -DY, 64, 33), "negative dy: ")
        up = t.a.compute_field_grid(X0, 780.3 + 32 * -DY, DX, DY, 64, 1)
        t.b.compute_accelerations()  # (keeps the twin in step)
        # (row 32 of the descending grid has the ascending grid's first y: same arithmetic)
        _assert_bits(down[2][32], up[2][0], "phi of the shared row")
    t.close()


def test_grid_point_on_a_body_gets_its_full_term():
    """soft2 = 1: the full self term, as compute_field and the checker give it."""
    arrs = _tree()
    cfg = make_cfg(theta=0.5, soft2=1.0)
    i = 777
    grid = (float(arrs[0][i]), float(arrs[1][i]), 0.7, 0.3, 5, 4)
    ax, ay, phi = _check(arrs, cfg, grid)
    assert np.all(np.isfinite(ax)) and np.all(np.isfinite(ay))
    # at least that body's own m / sqrt(soft2), which no neighbouring point reaches alone
    assert phi[0, 0] <= -(cfg["G"] * arrs[4][i])


def test_grid_point_on_a_body_without_softening():
    """soft2 = 0: NaN accelerations and -inf phi at that index only, excluded from the stats."""
    arrs = scenes.two_disks(100, 40)
    cfg = make_cfg(theta=0.5, soft2=0.0)
    probe = _engine(arrs, cfg)
    probe.compute_accelerations()  # (the positions the build leaves)
    x, y = probe.get_bodies()[:2]
    probe.close()
    t = _Twins(arrs, cfg)
    with np.errstate(all="ignore"):
        ax, ay, phi, s = t.check((float(x[3]), float(y[3]), 0.7, 0.3, 9, 5), want_stats=True)
    bad = np.zeros((5, 9), dtype=bool)
    bad[0, 0] = True
    assert np.array_equal(np.isnan(ax), bad) and np.array_equal(np.isnan(ay), bad)
    assert phi[0, 0] == -math.inf and np.all(np.isfinite(phi[~bad]))
    assert s.n_phi == 44 and s.n_acc == 44 and s.i_phi_min != 0 and s.i_a2_max != 0
    _assert_stats(s, (ax, ay, phi))
    t.close()


@pytest.mark.parametrize("name", ["jitter_306", "outside_153"])
def test_golden_scenes(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    w, h = cfg["width_px"], cfg["height_px"]
    _check(arrs, cfg, (-0.07 * w, -0.13 * h, 1.14 * w / 12, 1.26 * h / 6, 13, 7))


def test_massless_bodies():
    arrs = tuple(a.copy() for a in scenes.two_disks(600, 200))
    gone = np.random.default_rng(3).choice(800, 20, replace=False)
    arrs[4][gone] = 0.0
    _check(arrs, make_cfg(theta=0.5), (X0, Y0, 199.7, 131.3, 13, 7))
    # a grid point on a massless body
    g = gone[0]
    _check(arrs, make_cfg(theta=0.5), (float(arrs[0][g]), float(arrs[1][g]), 0.7, 0.3, 9, 2))


def test_one_body_and_empty_engines():
    one = (np.array([700.0]), np.array([300.0]), np.zeros(1), np.zeros(1), np.array([5.0]))
    ax, ay, phi = _check(one, make_cfg(theta=0.5), (700.0, 300.0, 37.7, -24.3, 9, 9))
    assert phi[0, 0] == -80.0 * 5.0 and ax[0, 0] == 0.0 and ay[0, 0] == 0.0
    empty = tuple(np.zeros(0) for _ in range(5))
    eng = _engine(empty, make_cfg(theta=0.5))
    ax, ay, phi, s = eng.compute_field_grid(X0, Y0, DX, DY, 13, 7, want_stats=True)
    _assert_bits(ax, np.zeros(91), "ax")
    _assert_bits(ay, np.zeros(91), "ay")
    _assert_bits(phi, -np.zeros(91), "phi")  # -(G * 0.0)
    assert s.n_phi == 91 and s.i_phi_min == 0 and s.phi_min == 0.0 and s.phi_max == 0.0
    assert s.n_acc == 91 and s.i_a2_max == 0 and s.a2_max == 0.0
    assert 0.0 < eng.field_grid_kernel_ms() < 1000.0
    eng.close()


# ---- stats -----------------------------------------------------------------------------------

def test_stats():
    eng = _engine(_tree(), make_cfg(theta=0.5))
    grid = (X0, Y0, 15.1, 8.3, 160, 96)
    ax, ay, phi, s = eng.compute_field_grid(*grid, want_stats=True)
    _assert_stats(s, (ax, ay, phi))
    assert s.n_phi == s.n_acc == 160 * 96 and s.phi_min < s.phi_max < 0.0 and s.a2_max > 0.0
    # all planes NULL: the same struct, and nothing else
    none = eng.compute_field_grid(*grid, want_accel=False, want_phi=False, want_stats=True)
    assert none[:3] == (None, None, None)
    assert stats_dict(none[3]) == stats_dict(s)
    # one plane NULL: the reduction still sees all three
    part = eng.compute_field_grid(*grid, want_phi=False, want_stats=True)
    assert part[2] is None and stats_dict(part[3]) == stats_dict(s)
    # stats NULL with the planes: the plain call
    _assert_field(eng.compute_field_grid(*grid), (ax, ay, phi))
    # a tie: dy = 0 makes every row equal, the first row's index answers; more points than one
    # reduction workgroup takes
    ax, ay, phi, s = eng.compute_field_grid(X0, 411.3, 7.03, 0.0, 341, 193, want_stats=True)
    _assert_bits(phi[192], phi[0], "equal rows")
    _assert_stats(s, (ax, ay, phi))
    assert 0 <= s.i_phi_min < 341 and 0 <= s.i_a2_max < 341
    eng.close()


# ---- state, usage, errors --------------------------------------------------------------------

def test_state_semantics_of_compute_accelerations():
    cfg = make_cfg(theta=0.5)
    a, b = _engine(_tree(), cfg), _engine(_tree(), cfg)
    a.compute_field_grid(X0, Y0, DX, DY, 64, 33)
    b.compute_accelerations()
    a.step(2)
    b.step(2)
    _assert_state(a, b.get_bodies())
    a.close()
    b.close()


def test_after_stepping():
    """After step(3) merges have shrunk N and the tree is the carried one."""
    arrs = scenes.config_scene("c1_baseline")
    cfg = make_cfg(theta=0.5)
    eng = _engine(arrs, cfg)
    eng.step(3)
    now = eng.get_bodies()
    grid = (X0, Y0, 199.7, 131.3, 13, 7)
    got = eng.compute_field_grid(*grid)
    want = checker_field(now, cfg, *grid_coords(*grid))
    _assert_field(got, want, "after step(3): ")
    _assert_state(eng, want[3])
    eng.close()


def test_repeatable_and_nullable_outputs():
    eng = _engine(_tree(), make_cfg(theta=0.5))
    grid = bh_amd.BhFieldGrid(X0, Y0, DX, DY, 13, 7)
    first = eng.compute_field_grid(X0, Y0, DX, DY, 64, 33)
    second = eng.compute_field_grid(X0, Y0, DX, DY, 64, 33)
    _assert_field(second, first)
    # a smaller grid after a larger one (the planes are larger than the call)
    full = eng.compute_field_grid(X0, Y0, DX, DY, 13, 7)
    _assert_field(full, [f[:7, :13] for f in first])
    for skip in range(3):
        out = [np.full(91, 7.0) for _ in range(3)]
        ptrs = [None if k == skip else out[k].ctypes.data_as(_D) for k in range(3)]
        rc = eng._lib.bh_compute_field_grid(eng._h, ctypes.byref(grid), *ptrs, None)
        assert rc == bh_amd.BH_OK
        for k in range(3):
            if k != skip:
                _assert_bits(out[k], full[k], f"output {k} without output {skip}")
    ax, ay, phi = eng.compute_field_grid(X0, Y0, DX, DY, 13, 7, want_accel=False)
    assert ax is None and ay is None
    _assert_bits(phi, full[2], "phi")
    assert eng._lib.bh_compute_field_grid(eng._h, ctypes.byref(grid), None, None, None,
                                          None) == bh_amd.BH_OK
    eng.close()


def test_timer_is_the_calls_own():
    eng = _engine(_tree(), make_cfg(theta=0.5))
    px, py = grid_coords(X0, Y0, DX, DY, 13, 7)
    assert eng.field_grid_kernel_ms() == 0.0
    eng.compute_field(px, py)
    assert eng.field_grid_kernel_ms() == 0.0
    eng.compute_field_grid(X0, Y0, DX, DY, 13, 7)
    ms = eng.field_grid_kernel_ms()
    assert 0.0 < ms < 1000.0
    field_ms = eng.field_kernel_ms()
    eng.compute_field(px, py)
    eng.compute_field_direct(px, py)
    eng.compute_potential()
    eng.force_error(np.arange(10))
    eng.compute_accelerations()
    eng.step(1)
    assert eng.field_grid_kernel_ms() == ms
    eng.compute_field_grid(X0, Y0, DX, DY, 13, 7, want_accel=False, want_phi=False,
                           want_stats=True)
    assert 0.0 < eng.field_grid_kernel_ms() < 1000.0
    assert field_ms > 0.0
    eng.close()


def test_invalid_arguments():
    eng = _engine(scenes.two_disks(100, 40), make_cfg(theta=0.5))
    lib = eng._lib
    ok = bh_amd.BhFieldGrid(X0, Y0, DX, DY, 13, 7)
    assert lib.bh_compute_field_grid(None, ctypes.byref(ok), None, None, None,
                                     None) == bh_amd.BH_E_INVALID
    assert lib.bh_compute_field_grid(eng._h, None, None, None, None, None) == bh_amd.BH_E_INVALID
    assert b"bh_compute_field_grid: g is NULL" in lib.bh_last_error(eng._h)
    cases = [(dict(nx=0), "nx and ny must be in 1..16384"),
             (dict(ny=0), "nx and ny must be in 1..16384"),
             (dict(nx=-5), "nx and ny must be in 1..16384"),
             (dict(nx=16385, ny=1), "nx and ny must be in 1..16384"),
             (dict(nx=1, ny=16385), "nx and ny must be in 1..16384"),
             (dict(nx=4097, ny=4096), "nx * ny must not exceed 1 << 24"),
             (dict(x0=math.nan), "x0, y0, dx and dy must be finite"),
             (dict(y0=math.inf), "x0, y0, dx and dy must be finite"),
             (dict(dx=-math.inf), "x0, y0, dx and dy must be finite"),
             (dict(dy=math.nan), "x0, y0, dx and dy must be finite")]
    for over, text in cases:
        kw = dict(x0=X0, y0=Y0, dx=DX, dy=DY, nx=13, ny=7)
        kw.update(over)
        with pytest.raises(bh_amd.BhError) as ei:
            eng.compute_field_grid(**kw)
        assert ei.value.rc == bh_amd.BH_E_INVALID, over
        assert "bh_compute_field_grid: " + text in str(ei.value), over
    assert eng.field_grid_kernel_ms() == 0.0  # refused before anything was launched
    ms = ctypes.c_double(1.0)
    assert lib.bh_field_grid_kernel_ms(None, ctypes.byref(ms)) == bh_amd.BH_E_INVALID
    assert lib.bh_field_grid_kernel_ms(eng._h, None) == bh_amd.BH_E_INVALID
    eng.close()


def test_async_guard():
    eng = _engine(scenes.two_disks(300, 100), make_cfg(theta=0.5))
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        with pytest.raises(bh_amd.BhError) as ei:
            eng.compute_field_grid(X0, Y0, DX, DY, 13, 7)
        assert ei.value.rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    assert eng.compute_field_grid(X0, Y0, DX, DY, 13, 7)[2].shape == (7, 13)
    eng.close()


def test_multi_handle_equals_single_engine(monkeypatch):
    """Every member builds, member 0 evaluates and answers: the planes, the stats and the state
    that follows equal the one-GPU engine's, before and after steps."""
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    cfg = make_cfg(theta=0.5)
    grid = (X0, Y0, DX, DY, 64, 33)
    one = _engine(_tree(), cfg)
    two = _engine(_tree(), cfg, devices=[0, 0])
    assert two.multi_world() == 2
    for rnd in range(2):
        got = two.compute_field_grid(*grid, want_stats=True)
        want = one.compute_field_grid(*grid, want_stats=True)
        _assert_field(got[:3], want[:3], f"round {rnd}: ")
        assert stats_dict(got[3]) == stats_dict(want[3])
        if rnd == 0:
            _assert_field(got[:3], _reference()[0][(64, 33)])
        one.step(2)
        two.step(2)
        _assert_state(two, one.get_bodies(), f"round {rnd}: ")
    logs = [two.member(r).collective_log() for r in range(2)]
    assert np.array_equal(logs[0], logs[1])
    assert two.field_grid_kernel_ms() > 0.0
    two.close()
    one.close()
