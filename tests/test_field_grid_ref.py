"""The grid field query (bh_compute_field_grid) on CPU: its host-only entry points, and the NumPy
statements of what the grid's points and the stats are.

`grid_coords` and `stats_rule` restate the header's definition; tests/test_gpu_field_grid.py
imports both and checks the engine against them and against the checker of
tests/test_field_ref.py.  `bodies_per_wave` / `waves_per_group` restate the traversal's launch
rules (traverse.hip), cross-checked here against bh_launch_plan wherever that reports them.
"""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bh_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")
VIEW_HPP = os.path.join(ROOT, "barnes-hut-n-body_amd", "csrc", "render_view.hpp")
SYMBOLS = ("bh_compute_field_grid", "bh_field_grid_of_view", "bh_field_grid_kernel_ms",
           "bh_field_grid_shape")
_I64P = ctypes.POINTER(ctypes.c_int64)


def grid_coords(x0, y0, dx, dy, nx, ny):
    """(px, py) of the grid's points, row-major (index r * nx + c): x0 + c * dx and y0 + r * dy,
    each one binary64 multiply and one binary64 add (NumPy rounds after each operation)."""
    cx = np.float64(x0) + np.arange(nx, dtype=np.float64) * np.float64(dx)
    cy = np.float64(y0) + np.arange(ny, dtype=np.float64) * np.float64(dy)
    px = np.ascontiguousarray(np.broadcast_to(cx[None, :], (ny, nx))).ravel()
    py = np.ascontiguousarray(np.broadcast_to(cy[:, None], (ny, nx))).ravel()
    return px, py


def stats_rule(ax, ay, phi):
    """struct bh_field_grid_stats as a dict, from the three planes alone: extremes under the
    order (value, row-major index) -- np.argmax of an equality mask is the first index."""
    ax, ay, phi = (np.asarray(a, dtype=np.float64).ravel() for a in (ax, ay, phi))
    out = dict(n_phi=0, i_phi_min=-1, phi_min=0.0, phi_max=0.0, n_acc=0, i_a2_max=-1, a2_max=0.0)
    fin = np.isfinite(phi)
    if fin.any():
        v = phi[fin]
        out["n_phi"] = int(fin.sum())
        out["phi_min"], out["phi_max"] = float(v.min()), float(v.max())
        out["i_phi_min"] = int(np.argmax(fin & (phi == v.min())))
    acc = np.isfinite(ax) & np.isfinite(ay)
    if acc.any():
        with np.errstate(over="ignore"):
            a2 = ax * ax + ay * ay  # two rounded products, one rounded sum
        out["n_acc"] = int(acc.sum())
        out["a2_max"] = float(a2[acc].max())
        out["i_a2_max"] = int(np.argmax(acc & (a2 == a2[acc].max())))
    return out


def stats_dict(s):
    return {name: getattr(s, name) for name, _ in bh_amd.BhFieldGridStats._fields_}


def bodies_per_wave(lanes):
    bpw = 64
    while bpw > 1 and (lanes + bpw - 1) // bpw < 1024:
        bpw //= 2
    return bpw


def waves_per_group(waves, bpw):
    if bpw < 64:
        return 1
    return 4 if waves >= 8192 else 8 if waves >= 1024 else 1


TILE_OF = {64: (8, 8), 32: (8, 4), 16: (4, 4), 8: (4, 2), 4: (2, 2), 2: (2, 1), 1: (1, 1)}


def shape_boundaries(nx, rows):
    """The ny in `rows` (ascending) at which field_grid_shape(nx, ny)[:3] differs from that of the
    ny before it."""
    shapes = [bh_amd.field_grid_shape(nx, ny)[:3] for ny in rows]
    return [rows[k] for k in range(1, len(rows)) if shapes[k] != shapes[k - 1]]


# ---- exports ---------------------------------------------------------------------------------

def test_header_declares_the_grid_symbols():
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = bh_amd.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert name in bh_amd.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "typedef struct bh_field_grid {" in code and "} bh_field_grid_stats;" in code
    # the call is in the list of calls refused between bh_step_begin and bh_step_end
    begin = txt[:txt.index("int bh_step_begin(")]
    assert "bh_compute_field_grid" in begin[begin.rindex("/*"):]
    assert ctypes.sizeof(bh_amd.BhFieldGrid) == 40 and ctypes.sizeof(bh_amd.BhFieldGridStats) == 56


# ---- bh_field_grid_shape ---------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", [(1, 1), (64, 1), (1, 65), (8, 8), (9, 9), (13, 7), (64, 33),
                                   (341, 3), (341, 4), (160, 96), (341, 192), (341, 193),
                                   (600, 200), (1024, 504), (1024, 505), (2400, 800),
                                   (16384, 1), (1, 16384), (16384, 1024), (4096, 4096)])
def test_shape_follows_the_traversal_rules(nx, ny):
    tw, th, wpb, tiles = bh_amd.field_grid_shape(nx, ny)
    n = nx * ny
    bpw = bodies_per_wave(n)
    assert (tw, th) == TILE_OF[bpw]
    assert tiles == -(-nx // tw) * -(-ny // th)
    assert tiles * tw * th >= n
    assert wpb == waves_per_group(tiles, bpw)
    plan = bh_amd.launch_plan(n) if n <= 1 << 22 else None
    if plan is not None and not plan["bfs"]:  # (the engine's own bodies_per_wave)
        assert plan["bpw"] == tw * th


def test_shape_changes_exactly_where_the_rules_change():
    # 341 columns: 3 * b rows are 1023 * b points, the largest grid that still gets b / 2 points
    # per wave (b points would make fewer than 1024 waves)
    rows = list(range(1, 201))
    want = [ny for ny in rows[1:] if bodies_per_wave(341 * ny) != bodies_per_wave(341 * (ny - 1))]
    assert want == [7, 13, 25, 49, 97, 193]
    assert shape_boundaries(341, rows) == want
    # 1024 columns of 8 x 8 tiles: 8192 tiles from row 505 on (4 waves per workgroup, from 8)
    assert shape_boundaries(1024, list(range(400, 600))) == [505]
    assert bh_amd.field_grid_shape(1024, 504)[2:] == (8, 128 * 63)
    assert bh_amd.field_grid_shape(1024, 505)[2:] == (4, 128 * 64)


def test_shape_refuses_bad_arguments():
    lib = bh_amd.load_library()
    out = np.zeros(4, dtype=np.int64)
    p = out.ctypes.data_as(_I64P)
    assert lib.bh_field_grid_shape(8, 8, None) == bh_amd.BH_E_INVALID
    for nx, ny in ((0, 8), (8, 0), (-1, 8), (16385, 1), (1, 16385), (4097, 4096), (16384, 1025)):
        assert lib.bh_field_grid_shape(nx, ny, p) == bh_amd.BH_E_INVALID, (nx, ny)
        with pytest.raises(bh_amd.BhError):
            bh_amd.field_grid_shape(nx, ny)
    assert lib.bh_field_grid_shape(16384, 1024, p) == bh_amd.BH_OK


# ---- bh_field_grid_of_view -------------------------------------------------------------------

@pytest.mark.parametrize("cell_px", [1, 4, 7])
def test_grid_of_view_closed_forms(cell_px):
    vx, vy, zoom, w, h = 3.1, -7.7, 1.3, 2399, 801
    g = bh_amd.field_grid_of_view(vx, vy, zoom, w, h, cell_px)
    assert (g.nx, g.ny) == (-(-w // cell_px), -(-h // cell_px))
    want = (vx + (0.5 * cell_px) / zoom, vy + (0.5 * cell_px) / zoom, cell_px / zoom,
            cell_px / zoom)
    got = (g.x0, g.y0, g.dx, g.dy)
    assert np.array_equal(np.array(got).view(np.int64), np.array(want).view(np.int64))
    # the grid's points are the centres of the pixel blocks, the last block clipped by the view
    px, _ = grid_coords(g.x0, g.y0, g.dx, g.dy, g.nx, 1)
    assert vx + (g.nx - 1) * cell_px / zoom < px[-1] < vx + w / zoom + 0.5 * cell_px / zoom


def test_grid_of_view_errors_are_the_views():
    texts = re.findall(r'return "(bh_view: [^"]+)"', open(VIEW_HPP).read())
    assert len(texts) == 4
    lib = bh_amd.load_library()
    bad = [dict(zoom=0.0), dict(zoom=math.inf), dict(heavy_mass=math.nan), dict(width=0),
           dict(height=16385), dict(width=16384, height=1025)]
    seen = set()
    for over in bad:
        kw = dict(view_x=0.0, view_y=0.0, zoom=1.0, width=100, height=50, cell_px=4)
        kw.update(over)
        with pytest.raises(bh_amd.BhError) as ei:
            bh_amd.field_grid_of_view(**kw)
        assert ei.value.rc == bh_amd.BH_E_INVALID
        hit = [t for t in texts if t in str(ei.value)]
        assert len(hit) == 1, (over, str(ei.value))
        seen.add(hit[0])
    assert seen == set(texts)
    for cell_px in (0, -3, 16385):
        with pytest.raises(bh_amd.BhError) as ei:
            bh_amd.field_grid_of_view(cell_px=cell_px)
        assert ei.value.rc == bh_amd.BH_E_INVALID and "cell_px must be in 1..16384" in str(ei.value)
    v = bh_amd.default_view()
    g = bh_amd.BhFieldGrid()
    assert lib.bh_field_grid_of_view(None, 4, ctypes.byref(g)) == bh_amd.BH_E_INVALID
    assert lib.bh_field_grid_of_view(ctypes.byref(v), 4, None) == bh_amd.BH_E_INVALID
    assert b"NULL" in lib.bh_last_error(None)
    # a success clears the text of the handle-less call
    assert lib.bh_field_grid_of_view(ctypes.byref(v), 4, ctypes.byref(g)) == bh_amd.BH_OK
    assert lib.bh_last_error(None) == b"null engine"
    assert (g.nx, g.ny) == (600, 200)


# ---- the NumPy statements --------------------------------------------------------------------

def test_grid_coords_are_two_rounded_operations():
    x0, y0, dx, dy, nx, ny = 3.1, -2.3, 0.7, -0.3, 13, 7
    px, py = grid_coords(x0, y0, dx, dy, nx, ny)
    assert px.shape == py.shape == (nx * ny,)
    fused = 0
    for r in range(ny):
        for c in range(nx):
            assert px[r * nx + c] == x0 + float(c) * dx and py[r * nx + c] == y0 + float(r) * dy
            # the exactly rounded x0 + c * dx (one rounding) differs somewhere on such a grid:
            # an FMA would show
            exact = float(Fraction(x0) + c * Fraction(dx))
            fused += exact != px[r * nx + c]
    assert fused > 0


def test_stats_rule():
    nan, inf = math.nan, math.inf
    phi = np.array([-1.0, -5.0, nan, -5.0, -inf, -0.5])
    ax = np.array([3.0, nan, 0.0, -4.0, 1.0, 4.0])
    ay = np.array([4.0, 0.0, 0.0, 3.0, inf, -3.0])
    s = stats_rule(ax, ay, phi)
    assert s == dict(n_phi=4, i_phi_min=1, phi_min=-5.0, phi_max=-0.5, n_acc=4, i_a2_max=0,
                     a2_max=25.0)
    s = stats_rule(np.full(3, nan), np.zeros(3), np.full(3, inf))
    assert s == dict(n_phi=0, i_phi_min=-1, phi_min=0.0, phi_max=0.0, n_acc=0, i_a2_max=-1,
                     a2_max=0.0)
    s = stats_rule(np.zeros((2, 3)), np.zeros((2, 3)), -np.zeros((2, 3)))  # an empty engine
    assert s["n_phi"] == 6 and s["i_phi_min"] == 0 and s["phi_min"] == 0.0
    assert s["n_acc"] == 6 and s["i_a2_max"] == 0 and s["a2_max"] == 0.0
