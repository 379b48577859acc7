"""The checker of bh_render_quads and its own cross-check, on CPU.

`quads_loop` is the literal per-cell loop of NBodyPanel.paintComponent's overlay (PNL:334-340):
for every cell of visitQuads, x = toInt(((cx - h) - view_x) * zoom), y likewise,
s = toInt(h * 2.0 * zoom) with Kotlin's Double.toInt(), then drawLine(x, y, x, y + s) and
drawLine(x, y, x + s, y) pixel by pixel under clipping, counting the draws per pixel.
`quads_ref` is the vectorised restatement of the contract in include/bh_engine.h: difference
arrays plus cumsum.  The two must agree byte for byte on the oracle's quads().
tests/test_gpu_render_quads.py checks the engine against `quads_ref`.
"""
import os
import re

import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from test_render_ref import VIEWS, kt_to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("x", "y", "vx", "vy", "m")

# (view_x, view_y, zoom, width, height)
WHOLE_ROOT = (-2.0, -802.0, 0.02, 64, 64)    # the root cell (1200, 400, 1202) is 49 x 49 pixels
CLOSE_UP = (1190.0, 395.0, 10.0, 128, 64)    # the top levels' lines are longer than the view
ODD_SIZES = [(0.0, 0.0, 0.05, 1, 1), (900.0, -300.0, 0.2, 5, 300), (-100.0, 350.0, 0.2, 300, 5),
             (-40.5, 13.25, 0.031, 37, 29)]
QUAD_VIEWS = list(VIEWS) + [WHOLE_ROOT, CLOSE_UP] + ODD_SIZES


def quads_loop(cx, cy, h, view_x=0.0, view_y=0.0, zoom=1.0, width=2400, height=800):
    """PNL:334-340, cell by cell and pixel by pixel: the line draws that cover each pixel."""
    lines = np.zeros((height, width), dtype=np.uint32)
    for i in range(len(cx)):
        qx, qy, qh = float(cx[i]), float(cy[i]), float(h[i])
        x = kt_to_int(((qx - qh) - view_x) * zoom)
        y = kt_to_int(((qy - qh) - view_y) * zoom)
        s = kt_to_int(qh * 2.0 * zoom)
        if 0 <= x < width:  # drawLine(x, y, x, y + s)
            for yy in range(max(y, 0), min(y + s, height - 1) + 1):
                lines[yy, x] += 1
        if 0 <= y < height:  # drawLine(x, y, x + s, y)
            for xx in range(max(x, 0), min(x + s, width - 1) + 1):
                lines[y, xx] += 1
    return lines


def to_int_vec(d):
    """Kotlin's Double.toInt() over an array, as int64."""
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros(d.shape, dtype=np.int64)
    ok = ~np.isnan(d)
    out[ok] = np.trunc(np.clip(d[ok], -2147483648.0, 2147483647.0)).astype(np.int64)
    return out


def quads_ref(cx, cy, h, view_x=0.0, view_y=0.0, zoom=1.0, width=2400, height=800):
    """The contract, vectorised: uint32 (height, width)."""
    cx, cy, h = (np.asarray(a, dtype=np.float64) for a in (cx, cy, h))
    with np.errstate(invalid="ignore", over="ignore"):
        x = to_int_vec(((cx - h) - view_x) * zoom)
        y = to_int_vec(((cy - h) - view_y) * zoom)
        s = to_int_vec(h * 2.0 * zoom)
    cold = np.zeros((height + 1, width), dtype=np.int64)
    r0, r1 = np.maximum(y, 0), np.minimum(y + s, height - 1)
    k = (x >= 0) & (x < width) & (r0 <= r1)
    np.add.at(cold, (r0[k], x[k]), 1)
    np.add.at(cold, (r1[k] + 1, x[k]), -1)
    rowd = np.zeros((height, width + 1), dtype=np.int64)
    c0, c1 = np.maximum(x, 0), np.minimum(x + s, width - 1)
    k = (y >= 0) & (y < height) & (c0 <= c1)
    np.add.at(rowd, (y[k], c0[k]), 1)
    np.add.at(rowd, (y[k], c1[k] + 1), -1)
    total = np.cumsum(cold, axis=0)[:height] + np.cumsum(rowd, axis=1)[:, :width]
    return total.astype(np.uint32)


def view_kw(view):
    return dict(zip(("view_x", "view_y", "zoom", "width", "height"), view))


def _oracle_quads(arrs, **kw):
    ref = oracle.Oracle(*arrs, **kw)
    q = ref.quads()
    ref.close()
    return q


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    p = z["params"]
    kw = dict(G=float(p[0]), dt=float(p[1]), theta=float(p[2]), soft2=float(p[3]),
              width_px=int(p[4]), height_px=int(p[5]), merge_max_mass=float(p[6]),
              merge_min_dist=float(p[7]))
    return tuple(z[f"init_{f}"] for f in FIELDS), kw


def outside_scene():
    """two_disks(100, 40) plus bodies outside the root cell (never inserted, BHA:126)."""
    arrs = scenes.two_disks(100, 40)
    ex = np.array([-3.0, 2403.0, 1200.0, 1200.0, -3.0])
    ey = np.array([400.0, 400.0, -803.0, 1603.0, np.nan])
    z = np.zeros(len(ex))
    return tuple(np.concatenate([a, b]) for a, b in zip(arrs, (ex, ey, z, z, np.ones(len(ex)))))


def close_pair(gap=5e-4):
    """Two bodies `gap` apart: one depth-J cell, the jitter replay."""
    x = np.array([700.5, 700.5 + gap])
    y = np.array([300.25, 300.25])
    z = np.zeros(2)
    return x, y, z, z.copy(), np.ones(2)


@pytest.fixture(scope="module")
def scene_quads():
    g_arrs, g_kw = _golden("jitter_306.npz")
    return {
        "two_disks": _oracle_quads(scenes.two_disks(300, 100)),
        "outside": _oracle_quads(outside_scene()),
        "close_pair": _oracle_quads(close_pair()),
        "jitter_306": _oracle_quads(g_arrs, **g_kw),
    }


@pytest.mark.parametrize("view", QUAD_VIEWS)
@pytest.mark.parametrize("scene", ["two_disks", "outside", "close_pair", "jitter_306"])
def test_checker_against_the_literal_loop(scene_quads, scene, view):
    cx, cy, h = scene_quads[scene]
    assert len(cx) >= 5
    got = quads_ref(cx, cy, h, *view)
    want = quads_loop(cx, cy, h, *view)
    assert got.dtype == want.dtype == np.uint32 and got.shape == (view[4], view[3])
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} pixels differ"
    print(f"{scene} {view}: {len(cx)} cells, {int(got.sum())} line pixels, max {got.max()}")


def test_close_pair_has_a_jitter_cell(scene_quads):
    """The pair shares its depth-J cell: cells below the depth whose h < 1e-3 exist."""
    _, _, h = scene_quads["close_pair"]
    assert h.min() < 1e-3 / 2


def test_close_up_lines_are_longer_than_the_view(scene_quads):
    cx, cy, h = scene_quads["two_disks"]
    lines = quads_ref(cx, cy, h, *CLOSE_UP)
    full_rows = np.flatnonzero((lines > 0).all(axis=1))
    full_cols = np.flatnonzero((lines > 0).all(axis=0))
    assert full_rows.size and full_cols.size  # a line that crosses the whole view each way


def test_root_alone():
    """From an empty list: s + 1 pixels on one row and on one column, the corner 2."""
    e = np.empty(0)
    cx, cy, h = _oracle_quads((e, e, e, e, e))
    assert (cx.tolist(), cy.tolist(), h.tolist()) == ([1200.0], [400.0], [1202.0])
    lines = quads_ref(cx, cy, h, *WHOLE_ROOT)
    s = kt_to_int(1202.0 * 2.0 * 0.02)
    assert s == 48
    want = np.zeros((64, 64), dtype=np.uint32)
    want[0, :s + 1] += 1
    want[:s + 1, 0] += 1
    assert want[0, 0] == 2 and np.array_equal(lines, want)
    assert np.array_equal(quads_loop(cx, cy, h, *WHOLE_ROOT), want)


@pytest.mark.parametrize("scene", ["two_disks", "close_pair", "jitter_306"])
def test_whole_root_sum(scene_quads, scene):
    """Nothing is clipped: every cell contributes its two lines of s + 1 pixels."""
    cx, cy, h = scene_quads[scene]
    lines = quads_ref(cx, cy, h, *WHOLE_ROOT)
    s = to_int_vec(h * 2.0 * WHOLE_ROOT[2])
    x = to_int_vec(((cx - h) - WHOLE_ROOT[0]) * WHOLE_ROOT[2])
    y = to_int_vec(((cy - h) - WHOLE_ROOT[1]) * WHOLE_ROOT[2])
    assert x.min() >= 0 and y.min() >= 0 and (x + s).max() < 64 and (y + s).max() < 64
    assert int(lines.sum()) == int((2 * (s + 1)).sum())


def test_half_a_pixel_left_of_the_view_draws_in_column_0():
    zoom = 0.25
    cx, cy, h = np.array([10.0 - 0.5 / zoom]), np.array([20.0]), np.array([8.0])
    # cx - h = view_x - half a pixel: tx = -0.5, toInt gives 0 (floor would give -1)
    view_x = (cx[0] - h[0]) + 0.5 / zoom
    lines = quads_ref(cx, cy, h, view_x, 0.0, zoom, 16, 16)
    assert kt_to_int(((cx[0] - h[0]) - view_x) * zoom) == 0
    y, s = kt_to_int((20.0 - 8.0) * zoom), kt_to_int(8.0 * 2.0 * zoom)
    assert (y, s) == (3, 4)
    assert lines[y:y + s + 1, 0].tolist() == [2, 1, 1, 1, 1]
    assert lines[y, :s + 1].tolist() == [2, 1, 1, 1, 1] and int(lines.sum()) == 10
    assert np.array_equal(lines, quads_loop(cx, cy, h, view_x, 0.0, zoom, 16, 16))


def test_nan_view_x_puts_every_vertical_line_in_column_0(scene_quads):
    cx, cy, h = scene_quads["two_disks"]
    _, view_y, zoom, width, height = WHOLE_ROOT
    lines = quads_ref(cx, cy, h, float("nan"), view_y, zoom, width, height)
    # the same picture as every cell's left edge on the view's origin
    assert np.array_equal(lines, quads_ref(h, cy, h, 0.0, view_y, zoom, width, height))
    s = to_int_vec(h * 2.0 * zoom)
    assert int(lines[:, 0].sum()) == int((s + 1).sum()) + len(h)  # vertical lines + row starts
    assert np.array_equal(lines, quads_loop(cx, cy, h, float("nan"), view_y, zoom, width, height))


def test_to_int_vec_is_kt_to_int():
    vals = [np.nan, -0.5, -0.999, -1.0, 7.999, 8.0, np.inf, -np.inf, 1e300, -1e300,
            2147483646.5, 2147483647.0, -2147483648.5, -2147483647.5]
    assert to_int_vec(vals).tolist() == [kt_to_int(v) for v in vals]


def test_header_declares_the_quad_render_calls():
    text = open(HEADER).read()
    for name in ("bh_render_quads", "bh_render_quads_kernel_ms"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in bh_amd.EXPORTED_SYMBOLS
    assert "bh_render_quads returns BH_E_STATE between bh_step_begin" in " ".join(text.split())\
        .replace(" * ", " ")
