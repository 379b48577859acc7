"""The Hilbert lane map made by run scatter equals the one made by the stable radix sort.

The map only groups bodies into waves, so it cannot be read back; what a traversal counts does
depend on it, wave by wave.  One engine is created with BH_LANE_ORDER_SORT=1 (the radix sort) and
one without (the run scatter), in one process, on the same scene: the visit-counting walk's
counters and per-body visits must be equal as integers, and the states bit-equal, after
reset_bodies (the in-line refresh) and again after step(7) (carried maps and a refresh beside a
traversal).  Every scene's property is checked on the CPU first, with a numpy restatement of the
key (tree_build.hip: hilbert16 of the Morton digits, >> BH_LANE_LO_BIT).
"""
import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from conftest import bits_equal

LANE_LO_BIT = 8
COUNTERS = ("waves", "wave_iters", "wave_blocks", "lane_visits", "lane_contrib")


# ---- the geometry and the sort key on the CPU ---------------------------------------------
def geometry(width, height):
    """(x0, y0, root side, J) as make_geometry (engine.cpp) derives them."""
    h = max(width, height) / 2.0 + 2.0
    J, hd = 0, h
    while hd >= 1e-3:
        hd /= 2.0
        J += 1
    return width / 2.0 - h, height / 2.0 - h, 2.0 * h, J


def in_root(x, y, width=2400, height=800):
    x0, y0, side, _ = geometry(width, height)
    return (x >= x0) & (x < x0 + side) & (y >= y0) & (y < y0 + side)


def hilbert(ix, iy, lv):
    """hilbert16 (tree_build.hip): the classic xy -> d over lv levels."""
    ix, iy = ix.astype(np.int64).copy(), iy.astype(np.int64).copy()
    h = np.zeros_like(ix)
    s = 1 << (lv - 1)
    while s > 0:
        rx, ry = ((ix & s) != 0).astype(np.int64), ((iy & s) != 0).astype(np.int64)
        h += s * s * ((3 * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        ix = np.where(flip, s - 1 - (ix & (s - 1)) + (ix & ~(s - 1)), ix)
        iy = np.where(flip, s - 1 - (iy & (s - 1)) + (iy & ~(s - 1)), iy)
        swap = ry == 0
        ix, iy = np.where(swap, iy, ix), np.where(swap, ix, iy)
        s >>= 1
    return h


def lane_keys(x, y, width=2400, height=800):
    """Sort key of every in-root body: the Hilbert index of its depth-min(J, 16) cell without
    its low LANE_LO_BIT bits."""
    x0, y0, side, J = geometry(width, height)
    lv = min(J, 16)
    ix = np.floor((x - x0) / side * (1 << lv)).astype(np.int64)
    iy = np.floor((y - y0) / side * (1 << lv)).astype(np.int64)
    return hilbert(ix, iy, lv) >> LANE_LO_BIT


def test_hilbert_restatement():
    # a Hilbert curve: a bijection whose consecutive cells share an edge, from (0, 0) to (max, 0)
    lv = 4
    iy, ix = np.divmod(np.arange(1 << (2 * lv)), 1 << lv)
    d = hilbert(ix, iy, lv)
    assert sorted(d) == list(range(1 << (2 * lv)))
    order = np.argsort(d)
    assert np.all(np.abs(np.diff(ix[order])) + np.abs(np.diff(iy[order])) == 1)
    assert (ix[order[0]], iy[order[0]]) == (0, 0)
    assert (ix[order[-1]], iy[order[-1]]) == ((1 << lv) - 1, 0)


# ---- the scenes ----------------------------------------------------------------------------
def uniform(n, seed, width=2400, height=800):
    r = np.random.default_rng(seed)
    x, y = r.uniform(0, width, n), r.uniform(0, height, n)
    vx, vy = r.uniform(-5, 5, n), r.uniform(-5, 5, n)
    return x, y, vx, vy, np.full(n, 0.5)


def scene_around_a_wave(n):
    arrs = uniform(n, 10 + n)
    assert len(arrs[0]) == n
    return arrs, {}


def scene_one_cell():
    # 3000 bodies inside one depth-12 Hilbert cell: one run, many workgroup chunks long
    n = 3000
    x0, y0, side, J = geometry(2400, 800)
    assert J >= 16
    w12 = side / 4096.0
    r = np.random.default_rng(3)
    x = x0 + (2000 + r.uniform(0.1, 0.9, n)) * w12
    y = y0 + (1700 + r.uniform(0.1, 0.9, n)) * w12
    keys = lane_keys(x, y)
    assert len(np.unique(keys)) == 1 and n > 10 * 256
    assert in_root(x, y).all()
    return (x, y, np.zeros(n), np.zeros(n), np.full(n, 0.5)), {}


def scene_sentinels():
    # 2000 bodies: 200 outside the root (sentinel keys: sort key 0xFFFFFF after the shift) and a
    # cluster in the corner cell where the Hilbert curve ends, whose real key is 0xFFFFFF too
    x0, y0, side, J = geometry(2400, 800)
    w12 = side / 4096.0
    r = np.random.default_rng(4)
    bx, by, _, _, _ = uniform(1500, 5)
    cx = x0 + side - r.uniform(0.1, 0.9, 300) * w12
    cy = y0 + r.uniform(0.1, 0.9, 300) * w12
    ox, oy = r.uniform(3000, 4000, 200), r.uniform(-3000, 3000, 200)
    x, y = np.concatenate([bx, ox, cx]), np.concatenate([by, oy, cy])
    perm = r.permutation(2000)
    x, y = x[perm], y[perm]
    inside = in_root(x, y)
    assert (~inside).sum() == 200
    keys = lane_keys(x[inside], y[inside])
    assert (keys == 0xFFFFFF).sum() == 300 and keys.max() == 0xFFFFFF
    assert (lane_keys(cx, cy) == 0xFFFFFF).all()
    n = len(x)
    return (x, y, np.zeros(n), np.zeros(n), np.full(n, 0.5)), {}


def scene_merges():
    # tombstones: the merge rule removes bodies within these 12 steps (the oracle agrees)
    import oracle
    arrs = scenes.two_disks(4000, 1000)
    ref = oracle.Oracle(*arrs, theta=0.5)
    ref.step(12)
    assert len(ref.get_bodies()[0]) < 5000
    return arrs, {"steps": 12, "merges": True}


def scene_many_cells():
    arrs = uniform(20_000, 6)
    coarse = np.unique(lane_keys(arrs[0], arrs[1]) >> 12)
    assert len(coarse) > 1000  # of 4096 coarse cells (the 2400 x 800 screen is a third of the root)
    return arrs, {}


def scene_short_keys(width):
    # a small root: J < 16, so the Hilbert index has fewer than 32 bits (J = 12: 16 key bits)
    _, _, _, J = geometry(width, width)
    assert J == {1: 12, 40: 15}[width]
    arrs = uniform(5000, 7, width, width)
    assert len(np.unique(lane_keys(arrs[0], arrs[1], width, width))) > 1000
    return arrs, {"width": width}


SCENES = {
    "n1": lambda: scene_around_a_wave(1),
    "n63": lambda: scene_around_a_wave(63),
    "n64": lambda: scene_around_a_wave(64),
    "n65": lambda: scene_around_a_wave(65),
    "one_cell_3000": scene_one_cell,
    "sentinel_collision": scene_sentinels,
    "merges_two_disks": scene_merges,
    "uniform_20000": scene_many_cells,
    "short_keys_J12": lambda: scene_short_keys(1),
    "short_keys_J15": lambda: scene_short_keys(40),
}


# ---- the comparison -------------------------------------------------------------------------
def engine_pair(monkeypatch, params):
    monkeypatch.setenv("BH_LANE_ORDER_SORT", "1")
    by_sort = bh_amd.Engine(params, device=0)
    monkeypatch.delenv("BH_LANE_ORDER_SORT")
    by_runs = bh_amd.Engine(params, device=0)
    return by_sort, by_runs


def assert_same_grouping(by_sort, by_runs, what):
    got = []
    for eng in (by_sort, by_runs):
        ax, ay, vis = eng.compute_accelerations(visits=True)
        got.append((ax, ay, vis, eng.traversal_counters(), eng.get_bodies()))
    (ax0, ay0, v0, c0, s0), (ax1, ay1, v1, c1, s1) = got
    for k in COUNTERS:
        assert c0[k] == c1[k], f"{what}: {k} {c0[k]} (sort) != {c1[k]} (run scatter)"
    assert c0["waves"] > 0
    assert np.array_equal(v0, v1), f"{what}: per-body visits differ"
    assert bits_equal(ax0, ax1) and bits_equal(ay0, ay1), f"{what}: accelerations differ"
    for a, b, name in zip(s0, s1, ("x", "y", "vx", "vy", "m")):
        assert bits_equal(a, b), f"{what}: state {name} differs"


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_has_its_property(name):
    SCENES[name]()  # (the scene's own assertions, on the CPU)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_run_scatter_groups_as_the_sort(name, monkeypatch):
    arrs, opt = SCENES[name]()
    width = opt.get("width")
    params = bh_amd.default_params(theta=0.5) if width is None else \
        bh_amd.default_params(theta=0.5, width_px=width, height_px=width)
    by_sort, by_runs = engine_pair(monkeypatch, params)
    try:
        for eng in (by_sort, by_runs):
            eng.reset_bodies(*arrs)
        assert_same_grouping(by_sort, by_runs, "after reset_bodies")
        for eng in (by_sort, by_runs):
            eng.step(opt.get("steps", 7))
        if opt.get("merges"):
            assert by_sort.num_bodies() < len(arrs[0])
        assert by_sort.num_bodies() == by_runs.num_bodies()
        assert_same_grouping(by_sort, by_runs, "after the steps")
    finally:
        by_sort.close()
        by_runs.close()
