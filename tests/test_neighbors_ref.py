"""The checker of the radius query (bh_find_neighbors) and the pruning bound, on CPU.

`candidates(arrs, cfg)` builds the reference's tree with oracle/py_oracle.py and lists the leaves
a walk reaches without passing a mass-0 node (test_potential_ref.leaves_preorder) as (caller
index, x, y) on the positions the build left; `brute(...)` applies the query's definition to them
with numpy: neighbour iff r >= 0 and dx*dx + dy*dy <= r*r, separate IEEE operations.  No tree
pruning is restated here.  tests/test_gpu_neighbors.py compares the engine exactly against it.

The bound: bh_neighbor_reach (host-only) must cover, on real trees, the distance from every
internal node's centre of mass to every such leaf under it -- the one check of the walk's
pruning that needs no GPU.
"""
import math
import os
import struct

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from test_potential_ref import build, cfg_from_golden, leaves_preorder, make_cfg, params_of
from oracle import py_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("x", "y", "vx", "vy", "m")


def candidates(arrs, cfg):
    """(idx, x, y, state, root): the candidate set S of the tree of `arrs`, ascending caller
    index, with the positions of the state after the build (the jitter has moved bodies)."""
    pe, root = build(arrs, cfg)
    index = {id(b): i for i, b in enumerate(pe.bodies)}
    idx = np.array(sorted(index[id(leaf.body)] for leaf in leaves_preorder(root)), dtype=np.int64)
    st = tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(pe))
    return idx, st[0][idx], st[1][idx], st, root


def brute(idx, x, y, px, py, r):
    """The query's definition on the candidates (idx ascending, x, y): dict of count, nearest,
    d2_nearest, offsets, indices.  r: one radius or one per probe."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    pr = np.broadcast_to(np.asarray(r, dtype=np.float64), px.shape)
    n = len(px)
    count = np.zeros(n, dtype=np.int64)
    nearest = np.full(n, -1, dtype=np.int64)
    d2n = np.full(n, np.inf)
    lists = [np.zeros(0, dtype=np.int64)]
    with np.errstate(all="ignore"):
        for lo in range(0, n if len(x) else 0, 2048):  # probes x candidates, a block at a time
            rows = slice(lo, min(lo + 2048, n))
            dx = x[None, :] - px[rows, None]
            dy = y[None, :] - py[rows, None]
            d2 = dx * dx + dy * dy
            rr = pr[rows, None]
            hit = (rr >= 0) & (d2 <= rr * rr)
            count[rows] = hit.sum(axis=1)
            lists.append(idx[np.nonzero(hit)[1]])  # row by row, each ascending
            # the first minimum among the hits is the lowest caller index; where that minimum
            # is +inf (r = +inf, a probe at 1e300) the first hit is
            masked = np.where(hit, d2, np.inf)
            k = np.argmin(masked, axis=1)
            k = np.where(np.isinf(masked[np.arange(len(k)), k]), np.argmax(hit, axis=1), k)
            some = count[rows] > 0
            nearest[rows] = np.where(some, idx[k], -1)
            d2n[rows] = np.where(some, d2[np.arange(len(k)), k], np.inf)
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    return dict(count=count, nearest=nearest, d2_nearest=d2n, offsets=offsets,
                indices=np.concatenate(lists))


def checker(arrs, cfg, px, py, r):
    """(brute's dict, state after the build) for the bodies `arrs`."""
    idx, x, y, st, _ = candidates(arrs, cfg)
    return brute(idx, x, y, px, py, r), st


def six_bodies():
    """0 alone; 1 and 2 a pair 20 apart; 3 outside the root cell; 4 of mass 0; 5 of negative
    mass (the root above it has positive mass)."""
    x = np.array([700.0, 1000.0, 1020.0, 5000.0, 1500.0, 300.0])
    y = np.array([300.0, 300.0, 300.0, 300.0, 600.0, 500.0])
    m = np.array([1.0, 2.0, 3.0, 1.0, 0.0, -3.0])
    return x, y, np.zeros(6), np.zeros(6), m


def _with_lsb(v, bit):
    """v, or its upper neighbour, whichever has `bit` as the last bit of its binary64 word."""
    if struct.unpack("<q", struct.pack("<d", v))[0] & 1 == bit:
        return v
    return math.nextafter(v, math.inf)


def jitter_pair(cfg):
    """six_bodies plus 6 and 7, placed in one depth-J cell of the root cell of `cfg` so that the
    jitter (BHA:146-151: +-1e-3 per axis, by the coordinate's last bit) moves 6 from the cell's
    lower-left corner into its upper-right child and 7 the other way: both are moved by the build
    and both stay in the tree, as leaves of depth J + 1.  (In tests/golden/jitter_306.npz every
    jittered body leaves its cell and is dropped from the tree.)"""
    h0 = max(cfg["width_px"], cfg["height_px"]) / 2.0 + 2.0
    J = next(d for d in range(64) if h0 / 2.0 ** d < 1e-3)
    w = 2.0 * h0 / 2.0 ** J  # 1e-3 <= w < 2e-3
    assert 1.12e-3 < w < 1.9e-3
    x0, y0 = cfg["width_px"] / 2.0 - h0, cfg["height_px"] / 2.0 - h0
    left = x0 + int((900.0 - x0) / w) * w
    low = y0 + int((300.0 - y0) / w) * w
    x, y, vx, vy, m = six_bodies()
    x = np.concatenate([x, [_with_lsb(left + 0.5e-4, 0), _with_lsb(left + w - 0.5e-4, 1)]])
    y = np.concatenate([y, [_with_lsb(low + 0.5e-4, 1), _with_lsb(low + w - 0.5e-4, 0)]])
    return x, y, np.zeros(8), np.zeros(8), np.concatenate([m, [2.0, 3.0]])


def test_jitter_pair_stays_in_the_tree():
    cfg = make_cfg()
    arrs = jitter_pair(cfg)
    idx, x, y, st, _ = candidates(arrs, cfg)
    assert idx.tolist() == [0, 1, 2, 5, 6, 7]
    assert (st[0][6:] - arrs[0][6:]).round(6).tolist() == [1e-3, -1e-3]
    assert (st[1][6:] - arrs[1][6:]).round(6).tolist() == [1e-3, -1e-3]
    # found where the build left them, not where they were
    got = brute(idx, x, y, np.concatenate([st[0][6:], arrs[0][6:]]),
                np.concatenate([st[1][6:], arrs[1][6:]]), 1e-5)
    assert got["count"].tolist() == [1, 1, 0, 0] and got["indices"].tolist() == [6, 7]


def test_checker_on_six_bodies():
    arrs = six_bodies()
    cfg = make_cfg()
    idx, x, y, st, _ = candidates(arrs, cfg)
    assert idx.tolist() == [0, 1, 2, 5]  # out of root and mass 0: not candidates
    for a, b in zip(st, arrs):
        assert np.array_equal(a, b)  # nothing here is jittered
    # r = 0 finds the coincident body, and only it
    got = brute(idx, x, y, [700.0], [300.0], 0.0)
    assert got["count"].tolist() == [1] and got["nearest"].tolist() == [0]
    assert got["d2_nearest"].tolist() == [0.0] and got["indices"].tolist() == [0]
    # ties go to the lower index
    got = brute(idx, x, y, [1010.0], [300.0], 10.0)
    assert got["count"].tolist() == [2] and got["nearest"].tolist() == [1]
    assert got["d2_nearest"].tolist() == [100.0] and got["indices"].tolist() == [1, 2]
    # ... and just below the tie's distance nothing is found
    got = brute(idx, x, y, [1010.0], [300.0], math.nextafter(10.0, 0.0))
    assert got["count"].tolist() == [0] and got["nearest"].tolist() == [-1]
    assert got["d2_nearest"].tolist() == [math.inf]
    # an out-of-root body and a mass-0 body are never found, a negative-mass body is
    got = brute(idx, x, y, [5000.0, 1500.0, 300.0], [300.0, 600.0, 500.0], 1.0)
    assert got["count"].tolist() == [0, 0, 1] and got["nearest"].tolist() == [-1, -1, 5]
    assert got["offsets"].tolist() == [0, 0, 0, 1]
    # +inf finds all of S; NaN and negative radii and NaN coordinates find nothing
    got = brute(idx, x, y, [0.0, 0.0, 0.0, math.nan], [0.0] * 4,
                np.array([math.inf, math.nan, -1.0, math.inf]))
    assert got["count"].tolist() == [4, 0, 0, 0]
    assert got["indices"].tolist() == [0, 1, 2, 5]


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    return tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z)


BOUND_SCENES = {
    "two_disks": lambda: (scenes.two_disks(600, 200), make_cfg(theta=0.5)),
    "jitter_306": lambda: _golden("jitter_306.npz"),
    "outside_153": lambda: _golden("outside_153.npz"),
    "screen_1920x1080": lambda: _golden("screen_1920x1080.npz"),
}


def reach_check(arrs, cfg):
    """Asserts the bound on the oracle's tree of `arrs`; returns (reachable leaves, internal
    nodes checked, (node, leaf) pairs checked, the deepest internal node checked)."""
    params = params_of(cfg)
    _, root = build(arrs, cfg)
    reach = [bh_amd.neighbor_reach(d, params) for d in range(40)]
    assert all(a > b > 0.0 for a, b in zip(reach, reach[1:]))
    ext = max(abs(root.quad.cx), abs(root.quad.cy)) + root.quad.h
    checked = [0, 0, 0]  # internal nodes, (node, leaf) pairs, deepest internal node

    def walk(node, depth):
        """The reachable leaves under `node` as (x, y); checks them against node's COM."""
        if node.mass == 0.0:
            return []
        if node.is_leaf():
            return [(node.body.x, node.body.y)] if node.body is not None else []
        under = []
        for c in node.children:
            under += walk(c, depth + 1)
        # the range of node masses the bound is stated for (include/bh_engine.h)
        assert 2.0 ** -900 <= node.mass < 1.7e308 / (8.0 * ext)
        checked[0] += 1
        checked[2] = max(checked[2], depth)
        for bx, by in under:
            dist = math.hypot(bx - node.comX, by - node.comY)
            assert dist <= reach[depth], (depth, dist, reach[depth])
            checked[1] += 1
        return under

    return (len(walk(root, 0)), *checked)


@pytest.mark.parametrize("scene", sorted(BOUND_SCENES))
def test_reach_covers_every_leaf_under_every_node(scene):
    leaves, nodes, pairs, _ = reach_check(*BOUND_SCENES[scene]())
    assert leaves > 100 and nodes > 50 and pairs > 500  # (the walk did look at real trees)


def test_reach_covers_jittered_leaves():
    """The depth-J node above two leaves that the jitter moved (and every node above it)."""
    cfg = make_cfg()
    leaves, nodes, pairs, deepest = reach_check(jitter_pair(cfg), cfg)
    assert leaves == 6 and deepest == 21 and nodes >= 21


def test_reach_refusals():
    lib = bh_amd.load_library()
    import ctypes
    p = bh_amd.default_params()
    out = ctypes.c_double(-7.0)
    assert lib.bh_neighbor_reach(None, 0, ctypes.byref(out)) == bh_amd.BH_E_INVALID
    assert lib.bh_neighbor_reach(ctypes.byref(p), 0, None) == bh_amd.BH_E_INVALID
    for depth in (-1, 40):
        assert lib.bh_neighbor_reach(ctypes.byref(p), depth, ctypes.byref(out)) \
            == bh_amd.BH_E_INVALID
    assert out.value == -7.0
    assert lib.bh_neighbor_reach(ctypes.byref(p), 39, ctypes.byref(out)) == bh_amd.BH_OK
    # the cell's diagonal is the bound's floor at every depth
    h0 = max(p.width_px, p.height_px) / 2.0 + 2.0
    for d in (0, 7, 39):
        assert bh_amd.neighbor_reach(d, p) > 2.0 * math.sqrt(2.0) * h0 / 2.0 ** d
