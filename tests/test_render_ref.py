"""The checker of bh_render_bodies and its own cross-check, on CPU.

`render_ref` is a vectorised numpy restatement of the contract in include/bh_engine.h: for body
i of the list, tx = (x_i - view_x) * zoom in binary64, sx = toInt(tx) with Kotlin's
Double.toInt() (NaN gives 0, otherwise truncation toward zero, saturating), drawn iff
0 <= sx < width and 0 <= sy < height; the owner of a pixel is the largest list index drawn on it
(np.maximum.at), counts the number drawn (np.bincount), pixels 1 (m[owner] < heavy_mass) or 2.
`render_loop` is the literal per-body loop of NBodyPanel.paintComponent (PNL:302-307) with a
`kt_to_int` helper; the two must agree byte for byte.  tests/test_gpu_render.py checks the engine
against `render_ref`.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import bh_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")
NONE = 0xFFFFFFFF

# (view_x, view_y, zoom, width, height)
VIEWS = [
    (0.0, 0.0, 0.05, 64, 48),
    (-40.5, 13.25, 0.031, 37, 29),
    (1100.3, 350.7, 0.25, 128, 64),
]


def kt_to_int(d: float) -> int:
    """Kotlin's Double.toInt()."""
    if d != d:
        return 0
    if d >= 2147483647.0:
        return 2147483647
    if d <= -2147483648.0:
        return -2147483648
    return int(d)  # truncation toward zero


def render_loop(x, y, m, view_x, view_y, zoom, width, height, heavy_mass=1000.0):
    """PNL:302-307, body by body: (pixels, owner, counts)."""
    pixels = np.zeros((height, width), dtype=np.uint8)
    owner = np.full((height, width), NONE, dtype=np.uint32)
    counts = np.zeros((height, width), dtype=np.uint32)
    for i in range(len(x)):
        sx = kt_to_int((float(x[i]) - view_x) * zoom)
        sy = kt_to_int((float(y[i]) - view_y) * zoom)
        if 0 <= sx < width and 0 <= sy < height:
            pixels[sy, sx] = 2 if float(m[i]) >= heavy_mass else 1
            owner[sy, sx] = i
            counts[sy, sx] += 1
    return pixels, owner, counts


def _axis(w, origin, zoom, size):
    """(drawn, pixel coordinate) along one axis."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(w, dtype=np.float64) - origin) * zoom
    nan = np.isnan(t)
    drawn = nan | ((t > -1.0) & (t < float(size)))
    s = np.trunc(np.where(drawn & ~nan, t, 0.0)).astype(np.int64)  # NaN -> 0
    return drawn, s


def render_ref(x, y, m, view_x=0.0, view_y=0.0, zoom=1.0, width=2400, height=800,
               heavy_mass=1000.0):
    """The contract, vectorised: (pixels uint8, owner uint32, counts uint32), (height, width)."""
    m = np.asarray(m, dtype=np.float64)
    dx, sx = _axis(x, view_x, zoom, width)
    dy, sy = _axis(y, view_y, zoom, height)
    idx = np.flatnonzero(dx & dy)
    p = sy[idx] * width + sx[idx]
    npix = width * height
    own = np.full(npix, -1, dtype=np.int64)
    np.maximum.at(own, p, idx)
    counts = np.bincount(p, minlength=npix).astype(np.uint32)
    lit = own >= 0
    pixels = np.zeros(npix, dtype=np.uint8)
    pixels[lit] = np.where(m[own[lit]] >= heavy_mass, 2, 1)
    owner = np.where(lit, own, NONE).astype(np.uint32)
    shape = (height, width)
    return pixels.reshape(shape), owner.reshape(shape), counts.reshape(shape)


def edge_bodies(n, view, seed=7):
    """n bodies around `view`: a uniform cloud a quarter of the view wider than it on every side,
    a clump that shares a few pixels, masses on both sides of the colour threshold, and the
    coordinates on which toInt and the bounds test can go wrong.  Returns (x, y, vx, vy, m) and
    the indices of the special bodies by name."""
    view_x, view_y, zoom, width, height = view
    rng = np.random.default_rng(seed)
    span_x, span_y = width / zoom, height / zoom
    x = view_x + rng.uniform(-0.25, 1.25, n) * span_x
    y = view_y + rng.uniform(-0.25, 1.25, n) * span_y
    k = n // 3
    x[:k] = view_x + 0.5 * span_x + rng.normal(0.0, 1.5 / zoom, k)
    y[:k] = view_y + 0.5 * span_y + rng.normal(0.0, 1.5 / zoom, k)
    m = rng.choice(np.array([0.5, 999.9999, 1000.0, 5000.0]), n)
    inside_x, inside_y = view_x + 0.3 * span_x, view_y + 0.6 * span_y
    special = {
        "nan_x": (np.nan, inside_y), "nan_y": (inside_x, np.nan), "nan_xy": (np.nan, np.nan),
        "pinf_x": (np.inf, inside_y), "ninf_x": (-np.inf, inside_y),
        "pinf_y": (inside_x, np.inf), "ninf_y": (inside_x, -np.inf),
        "big_x": (1e300, inside_y), "nbig_x": (-1e300, inside_y),
        "big_y": (inside_x, 1e300), "nbig_y": (inside_x, -1e300),
        "half_left": (view_x - 0.5 / zoom, inside_y),
        "half_above": (inside_x, view_y - 0.5 / zoom),
        "right_edge": (view_x + width / zoom, inside_y),
        "bottom_edge": (inside_x, view_y + height / zoom),
        "light": (inside_x, inside_y), "heavy": (inside_x, inside_y),
    }
    where = {}
    slots = np.linspace(n // 7, n - 1, len(special)).astype(int)  # spread, the last one at n - 1
    for slot, (name, (sx, sy)) in zip(slots, special.items()):
        x[slot], y[slot] = sx, sy
        where[name] = int(slot)
    m[where["light"]] = 999.9999
    m[where["heavy"]] = 1000.0
    z = np.zeros(n)
    return (x, y, z.copy(), z.copy(), m), where


@pytest.mark.parametrize("view", VIEWS)
def test_checker_against_the_literal_loop(view):
    (x, y, _, _, m), where = edge_bodies(5000, view)
    view_x, view_y, zoom, width, height = view
    got = render_ref(x, y, m, *view)
    want = render_loop(x, y, m, *view)
    for name, a, b in zip(("pixels", "owner", "counts"), got, want):
        assert a.dtype == b.dtype and a.shape == (height, width)
        assert np.array_equal(a, b), f"{name}: {np.count_nonzero(a != b)} pixels differ"
    pixels, owner, counts = got
    print(f"view {view}: {np.count_nonzero(pixels)} lit pixels, up to {counts.max()} per pixel")
    assert counts.sum() < 5000 and counts.max() > 1  # some outside, some share a pixel
    assert np.array_equal(counts > 0, pixels > 0)
    assert np.array_equal(owner != NONE, pixels > 0)
    # NaN lands in column / row 0; truncation is not floor; the far edge is outside
    row = kt_to_int((y[where["nan_x"]] - view_y) * zoom)
    col = kt_to_int((x[where["nan_y"]] - view_x) * zoom)
    assert counts[row, 0] >= 2 and counts[0, col] >= 2 and counts[0, 0] >= 1
    for name in ("pinf_x", "ninf_x", "pinf_y", "ninf_y", "big_x", "nbig_x", "big_y", "nbig_y"):
        i = where[name]
        assert not np.any(owner == i)
    # the last special body is the last of the list: it owns its pixel, and it is heavy
    i = where["heavy"]
    assert i == 4999 and pixels[owner == i].tolist() == [2]
    assert m[where["light"]] == 999.9999 and where["light"] < i


def test_nan_left_out_would_disagree():
    """The contract spells NaN out because a checker that drops NaN bodies disagrees."""
    view = VIEWS[0]
    (x, y, _, _, m), _ = edge_bodies(5000, view)
    keep = ~(np.isnan(x) | np.isnan(y))
    a = render_ref(x, y, m, *view)[2]
    b = render_ref(x[keep], y[keep], m[keep], *view)[2]
    assert a.sum() == b.sum() + 3


def test_truncation_known_answers():
    for d, want in ((np.nan, 0), (-0.5, 0), (-0.999, 0), (-1.0, -1), (7.999, 7), (8.0, 8),
                    (np.inf, 2147483647), (-np.inf, -2147483648), (1e300, 2147483647),
                    (-1e300, -2147483648), (2147483646.5, 2147483646)):
        assert kt_to_int(d) == want
    x = np.array([-0.5, 8.0, 3.0, 3.0])
    y = np.array([1.0, 1.0, 2.0, 2.0])
    m = np.array([1.0, 1.0, 1000.0, 1.0])
    pixels, owner, counts = render_ref(x, y, m, width=8, height=4)
    assert pixels[1, 0] == 1 and owner[1, 0] == 0  # tx = -0.5: column 0
    assert counts[1].sum() == 1                     # tx = width: not drawn
    assert pixels[2, 3] == 1 and owner[2, 3] == 3 and counts[2, 3] == 2  # heavy then light
    pixels, owner, _ = render_ref(x, y, m[[0, 1, 3, 2]], width=8, height=4)
    assert pixels[2, 3] == 2 and owner[2, 3] == 3  # light then heavy


def test_empty_list():
    e = np.empty(0)
    pixels, owner, counts = render_ref(e, e, e, width=5, height=3)
    assert not pixels.any() and not counts.any() and np.all(owner == NONE)


def test_view_struct_and_defaults():
    """BhView mirrors struct bh_view; bh_default_view needs no device."""
    assert ctypes.sizeof(bh_amd.BhView) == 40
    v = bh_amd.default_view()
    assert (v.view_x, v.view_y, v.zoom, v.width, v.height, v.heavy_mass) == \
        (0.0, 0.0, 1.0, 2400, 800, 1000.0)
    bh_amd.load_library().bh_default_view(None)  # NULL is ignored


def test_header_declares_the_render_calls():
    text = open(HEADER).read()
    for name in ("bh_default_view", "bh_render_bodies", "bh_render_kernel_ms"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in bh_amd.EXPORTED_SYMBOLS
    assert "bh_compute_diagnostics and bh_render_bodies return BH_E_STATE" in text
