"""GPU: bh_render_bodies / bh_render_kernel_ms / PhysicsEngine.render.

Every image check is byte-exact on all three planes (pixels, owner, counts) against the checker
of tests/test_render_ref.py applied to what get_bodies() returns from the same engine.
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from conftest import bits_equal
from test_render_ref import NONE, VIEWS, edge_bodies, render_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("x", "y", "vx", "vy", "m")
SMALL = dict(view_x=0.0, view_y=0.0, zoom=0.05, width=64, height=48)
DEFAULT = dict(view_x=0.0, view_y=0.0, zoom=1.0, width=2400, height=800)
CLOSE_UP = dict(view_x=1200.0, view_y=400.0, zoom=4.0, width=128, height=64)  # first disk's centre


def _engine(arrs, **kw):
    params = bh_amd.default_params(theta=kw.pop("theta", 0.5))
    eng = bh_amd.Engine(params, **(kw or {"device": 0}))
    eng.reset_bodies(*arrs)
    return eng


def _same(got, want, what):
    for name, a, b in zip(("pixels", "owner", "counts"), got, want):
        if a is None:
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} {a.dtype} {a.shape}"
        bad = np.argwhere(a != b)
        assert bad.size == 0, (f"{what}: {name} differs on {len(bad)} pixels, first (row, col) "
                               f"{bad[:3].tolist()}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}")


def _check(eng, what="image", **view):
    """All three planes against the checker over the engine's own get_bodies()."""
    x, y, _, _, m = eng.get_bodies()
    got = eng.render_bodies(owner=True, counts=True, **view)
    hm = {k: v for k, v in view.items() if v is not None}
    hm.setdefault("width", eng.params.width_px)
    hm.setdefault("height", eng.params.height_px)
    _same(got, render_ref(x, y, m, **hm), what)
    return got


def test_known_answer():
    """Two bodies on one pixel in both list orders, tx = -0.5 (column 0), tx = width (not drawn)."""
    x = np.array([-0.5, 8.0, 3.0, 3.0])
    y = np.array([1.0, 1.0, 2.0, 2.0])
    z = np.zeros(4)
    for m, colour in ((np.array([1.0, 1.0, 1000.0, 1.0]), 1),    # heavy then light
                      (np.array([1.0, 1.0, 1.0, 1000.0]), 2)):   # light then heavy
        eng = _engine((x, y, z, z, m))
        pixels, owner, counts = _check(eng, width=8, height=4)
        want_p = np.zeros((4, 8), dtype=np.uint8)
        want_o = np.full((4, 8), NONE, dtype=np.uint32)
        want_c = np.zeros((4, 8), dtype=np.uint32)
        want_p[1, 0], want_o[1, 0], want_c[1, 0] = 1, 0, 1
        want_p[2, 3], want_o[2, 3], want_c[2, 3] = colour, 3, 2
        _same((pixels, owner, counts), (want_p, want_o, want_c), "known answer")
        eng.close()


@pytest.mark.parametrize("view", VIEWS)
def test_edge_coordinates_before_any_step(view):
    """NaN, +-inf, +-1e300, half a pixel outside, exactly on the far edge: a render only, no
    build is asked of this engine."""
    arrs, where = edge_bodies(5000, view)
    eng = _engine(arrs)
    keys = dict(zip(("view_x", "view_y", "zoom", "width", "height"), view))
    _, owner, counts = _check(eng, **keys)
    assert counts[0, 0] >= 1 and owner[0, 0] >= where["nan_xy"]
    for name, a, b in zip(FIELDS, eng.get_bodies(), arrs):
        assert bits_equal(a, b), name
    eng.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130, 5000])
def test_sizes(n):
    if n == 5000:
        arrs = tuple(np.concatenate([a, a + 3.0, a[:1000] + 7.0])
                     for a in scenes.config_scene("c1_baseline"))
    else:
        arrs = tuple(a[:n].copy() for a in scenes.two_disks(100, 40))
    assert len(arrs[0]) == n
    eng = _engine(arrs)
    pixels, owner, counts = _check(eng, **SMALL)
    assert (counts.sum() > 0) == (n > 0)
    if n == 0:
        assert not pixels.any() and np.all(owner == NONE)
    if n == 5000:
        assert counts.max() > 1  # many bodies share a pixel
    eng.close()


def test_contention():
    n = 4096
    z = np.zeros(n)
    x, y = np.full(n, 700.5), np.full(n, 300.25)
    m = np.ones(n)
    m[-1] = 2000.0
    eng = _engine((x, y, z, z, m))
    pixels, owner, counts = _check(eng, **SMALL)
    assert (pixels[15, 35], owner[15, 35], counts[15, 35]) == (2, 4095, 4096)
    assert counts.sum() == 4096
    x[n // 2:] += 20.0  # the second half one pixel to the right
    eng.reset_bodies(x, y, z, z, m)
    pixels, owner, counts = _check(eng, **SMALL)
    assert (pixels[15, 35], owner[15, 35], counts[15, 35]) == (1, 2047, 2048)
    assert (pixels[15, 36], owner[15, 36], counts[15, 36]) == (2, 4095, 2048)
    x[::2] -= 20.0  # alternating lanes on the two pixels: equal pixels that are not neighbours
    eng.reset_bodies(x, y, z, z, m)
    _check(eng, **SMALL)
    eng.close()


def test_after_stepping():
    """Slots in Morton order, merges behind, and a pre-built tree carried into the next call."""
    eng = _engine(scenes.two_disks(1500, 500))
    eng.step(3)
    _, _, counts = _check(eng, "default view", **DEFAULT)
    assert 0 < counts.sum() <= eng.num_bodies() <= 2000
    _, _, counts = _check(eng, "close-up", **CLOSE_UP)
    assert 0 < counts.sum() < eng.num_bodies()
    _check(eng, "engine's own size", zoom=0.5)  # width, height: the params' width_px, height_px
    eng.close()


def test_follows_get_bodies_not_the_carried_trees_jitter():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    p = z["params"]
    params = bh_amd.default_params(G=float(p[0]), dt=float(p[1]), theta=float(p[2]),
                                   soft2=float(p[3]), width_px=int(p[4]), height_px=int(p[5]),
                                   merge_max_mass=float(p[6]), merge_min_dist=float(p[7]))
    eng = bh_amd.Engine(params, device=0)
    eng.reset_bodies(*[z[f"init_{f}"] for f in FIELDS])
    eng.step(1)
    w, h = int(p[4]), int(p[5])
    _check(eng, "whole root", width=w, height=h)
    # what the next build's jitter would make of the visible list (a build on a second engine),
    # and a view fine enough to tell the two apart: four pixels per jitter displacement
    seen = eng.get_bodies()
    probe = bh_amd.Engine(params, device=0)
    probe.reset_bodies(*seen)
    probe.compute_accelerations()
    jit = probe.get_bodies()
    probe.close()
    moved = np.flatnonzero((jit[0] != seen[0]) | (jit[1] != seen[1]))
    print(f"{moved.size} bodies jittered by the build that follows the step")
    if moved.size:
        j = int(moved[0])
        d = max(abs(jit[0][j] - seen[0][j]), abs(jit[1][j] - seen[1][j]))
        zoom = 4.0 / d
        fine = dict(view_x=float(seen[0][j]) - 32.0 / zoom, view_y=float(seen[1][j]) - 16.0 / zoom,
                    zoom=zoom, width=64, height=32)
        got = _check(eng, "fine", **fine)
        other = render_ref(jit[0], jit[1], jit[4], **fine)
        assert any(not np.array_equal(a, b) for a, b in zip(got, other))
    eng.close()


def test_no_side_effect():
    arrs = scenes.two_disks(1500, 500)
    a, b = _engine(arrs), _engine(arrs)
    a.step(2)
    b.step(2)
    before = a.get_bodies()
    first = a.render_bodies(owner=True, counts=True, **DEFAULT)
    second = a.render_bodies(owner=True, counts=True, **DEFAULT)
    _same(second, first, "second render")
    for name, u, v in zip(FIELDS, a.get_bodies(), before):
        assert bits_equal(u, v), f"{name} after a render"
    a.step(2)
    b.step(2)  # (no render on this engine before its steps)
    for name, u, v in zip(FIELDS, a.get_bodies(), b.get_bodies()):
        assert bits_equal(u, v), f"{name} two steps after the renders"
    _same(b.render_bodies(owner=True, counts=True, **DEFAULT),
          a.render_bodies(owner=True, counts=True, **DEFAULT), "two engines, one list")
    a.close()
    b.close()


def test_changing_the_view_size_between_calls():
    eng = _engine(scenes.two_disks(1500, 500))
    eng.step(1)
    for view in (DEFAULT, SMALL, DEFAULT, dict(SMALL, width=37, height=29), SMALL):
        _check(eng, f"{view['width']}x{view['height']}", **view)
    eng.close()


def test_null_planes():
    eng = _engine(scenes.two_disks(1500, 500))
    eng.step(1)
    full = eng.render_bodies(owner=True, counts=True, **SMALL)
    for flags in itertools.product((False, True), repeat=3):
        got = eng.render_bodies(pixels=flags[0], owner=flags[1], counts=flags[2], **SMALL)
        if flags == (True, False, False):
            got = (got, None, None)  # pixels alone comes back bare
        assert [g is not None for g in got] == list(flags)
        _same(got, full, f"planes {flags}")
    _same(eng.render_bodies(owner=True, counts=True, **SMALL), full, "full again")
    eng.close()


def test_mirror_and_async():
    eng = _engine(scenes.two_disks(300, 100))
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        with pytest.raises(bh_amd.BhError) as ei:
            eng.render_bodies(**SMALL)
        assert ei.value.rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    _check(eng, **SMALL)
    x, y, _, _, m = (np.array(a) for a in eng.map_bodies())
    _same(eng.render_bodies(owner=True, counts=True, **SMALL), render_ref(x, y, m, **SMALL),
          "against the mirror")
    eng.close()


def test_multi_handle_equals_single_engine(monkeypatch):
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    arrs = scenes.two_disks(1500, 500)
    one, two = _engine(arrs), _engine(arrs, devices=[0, 0])
    assert two.multi_world() == 2
    one.step(2)
    two.step(2)
    want = _check(one, **SMALL)
    _same(_check(two, **SMALL), want, "multi handle")
    assert two.render_kernel_ms() > 0.0
    two.close()
    one.close()


@pytest.mark.parametrize("bad", [
    dict(zoom=0.0), dict(zoom=-1.0), dict(zoom=float("nan")), dict(zoom=float("inf")),
    dict(width=0), dict(width=16385), dict(height=0), dict(height=16385),
    dict(width=16384, height=1025), dict(heavy_mass=float("nan")),
])
def test_invalid_arguments(bad):
    eng = _engine(scenes.two_disks(100, 40))
    with pytest.raises(bh_amd.BhError) as ei:
        eng.render_bodies(**dict(SMALL, **bad))
    assert ei.value.rc == bh_amd.BH_E_INVALID
    assert eng._lib.bh_last_error(eng._h).decode().startswith("bh_view:")
    _check(eng, **SMALL)  # the engine is as usable as before
    eng.close()


def test_null_engine_or_view(engine_lib):
    eng = _engine(scenes.two_disks(100, 40))
    v = bh_amd.default_view()
    assert engine_lib.bh_render_bodies(None, ctypes.byref(v), None, None, None) == \
        bh_amd.BH_E_INVALID
    assert engine_lib.bh_render_bodies(eng._h, None, None, None, None) == bh_amd.BH_E_INVALID
    assert engine_lib.bh_render_bodies(eng._h, ctypes.byref(v), None, None, None) == bh_amd.BH_OK
    eng.close()


def test_render_kernel_ms():
    eng = _engine(scenes.two_disks(1500, 500))
    assert eng.render_kernel_ms() == 0.0
    eng.render_bodies(**DEFAULT)
    assert 0.0 < eng.render_kernel_ms() < 1000.0
    eng.close()


def test_physics_engine_render_after_an_edit(monkeypatch):
    monkeypatch.setattr(bh_amd.Config, "theta", 0.5)
    x, y, vx, vy, m = scenes.two_disks(300, 100)
    bodies = [bh_amd.Body(*map(float, t)) for t in zip(x, y, vx, vy, m)]
    pe = bh_amd.PhysicsEngine(bodies)
    pe.step()

    def want():
        bs = pe.get_bodies()
        return render_ref(np.array([b.x for b in bs]), np.array([b.y for b in bs]),
                          np.array([b.m for b in bs]), **SMALL)

    _same(pe.render(owner=True, counts=True, **SMALL), want(), "after a step")
    last = bodies[-1]
    last.x, last.y, last.m = 30.0, 50.0, 2500.0  # the caller edits a Body between frames
    pixels, owner, counts = pe.render(owner=True, counts=True, **SMALL)
    _same((pixels, owner, counts), want(), "after the edit")
    assert (pixels[2, 1], owner[2, 1], counts[2, 1]) == (2, len(bodies) - 1, 1)
    assert pe.render(**SMALL).dtype == np.uint8
