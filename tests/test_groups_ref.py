"""The checker of the friends-of-friends group finder (bh_find_groups), on CPU.

The candidate set S and the state after the build come from test_neighbors_ref.candidates (the
oracle's tree).  `fof_all_pairs` is the definition in numpy: the full `d2 <= link*link` matrix and
a breadth-first sweep of its components; `fof_binned` finds the same pairs through a cell-binned
search (cells of side >= link, the 9 neighbouring cells, the exact test on the candidates) and
joins them with a vectorised union-find, for tens of thousands of bodies.  `catalogue` applies the
definition of members, groups, the two-level sums and the summary to a label array.  No tree
walk and no pruning is restated here.  tests/test_gpu_groups.py compares the engine exactly
against it.

Also here: the host-side ABI checks that need no GPU.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from test_neighbors_ref import FIELDS, candidates, jitter_pair, six_bodies
from test_potential_ref import cfg_from_golden, make_cfg

LINKS = (0.0, 1.0, 4.0, 8.0, 20.0, 50.0, math.inf)
BLOCK = 256  # members per block of a group's two-level sums (include/bh_engine.h)


def link_matrix(x, y, link):
    """adj[a, b] = dx*dx + dy*dy <= link*link with dx = x_a - x_b, separate IEEE operations."""
    with np.errstate(all="ignore"):
        dx = x[:, None] - x[None, :]
        dy = y[:, None] - y[None, :]
        return dx * dx + dy * dy <= link * link


def fof_all_pairs(idx, x, y, link):
    """Per candidate (idx: caller indices, x, y) the label of its group: the smallest caller
    index of its connected component of the full link matrix."""
    n = len(idx)
    adj = link_matrix(x, y, link)
    label = np.full(n, -1, dtype=np.int64)
    for seed in range(n):
        if label[seed] >= 0:
            continue
        seen = np.zeros(n, dtype=bool)
        seen[seed] = True
        frontier = np.array([seed])
        while frontier.size:
            reach = adj[frontier].any(axis=0) & ~seen
            seen |= reach
            frontier = np.flatnonzero(reach)
        label[seen] = idx[seen].min()
    return label


def binned_pairs(x, y, link):
    """(a, b), a != b: every linked pair of the candidates, both ways, through cells of side
    >= link and their 9 neighbours; the test itself is the definition's."""
    n = len(x)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    x0, y0 = x.min(), y.min()
    span = max(x.max() - x0, y.max() - y0, 1.0)
    side = max(link, span / 512.0)  # >= link; no more than 513 cells per axis
    if not math.isfinite(side):
        cx = cy = np.zeros(n, dtype=np.int64)
    else:
        cx = np.floor((x - x0) / side).astype(np.int64)
        cy = np.floor((y - y0) / side).astype(np.int64)
    W = int(cx.max()) + 3  # a column of empty cells on either side: no wrap-around
    cell = (cy + 1) * W + (cx + 1)
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    aa, bb = [], []
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            want = sc + oy * W + ox
            lo = np.searchsorted(sc, want, side="left")
            cnt = np.searchsorted(sc, want, side="right") - lo
            a = np.repeat(np.arange(n), cnt)
            within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            aa.append(order[a])
            bb.append(order[np.repeat(lo, cnt) + within])
    a, b = np.concatenate(aa), np.concatenate(bb)
    with np.errstate(all="ignore"):
        dx, dy = x[a] - x[b], y[a] - y[b]
        hit = (dx * dx + dy * dy <= link * link) & (a != b)
    return a[hit], b[hit]


def fof_binned(idx, x, y, link):
    """fof_all_pairs' answer through binned_pairs and a union-find (hook the higher root under
    the lower, compress, until no pair joins two roots)."""
    n = len(idx)
    a, b = binned_pairs(x, y, link)
    parent = np.arange(n)
    while True:
        pa, pb = parent[a], parent[b]
        open_ = pa != pb
        if not open_.any():
            break
        np.minimum.at(parent, np.maximum(pa, pb)[open_], np.minimum(pa, pb)[open_])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    low = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(low, parent, idx)
    return low[parent]


def labels_of(n_bodies, idx, per_candidate):
    """The call's label array: per body of the list, -1 for a body not in S."""
    label = np.full(n_bodies, -1, dtype=np.int64)
    label[idx] = per_candidate
    return label


def _seq(a):
    """The sequential sum of `a` in order, from +0.0."""
    return np.cumsum(np.concatenate([[0.0], a]))[-1]


def two_level(terms):
    """Blocks of 256 summed in order from +0.0, then the partials in order from +0.0."""
    return _seq(np.array([_seq(terms[k:k + BLOCK]) for k in range(0, len(terms), BLOCK)]))


def catalogue(label, state, min_members):
    """dict(label, members, groups, summary) of a label array on the state after the build
    (x, y, vx, vy, m in caller order).  groups: bh_amd.GROUP_DTYPE records; summary: the six
    fields of bh_groups_summary."""
    x, y, vx, vy, m = state
    n = len(label)
    in_s = np.flatnonzero(label >= 0)
    members = in_s[np.lexsort((in_s, label[in_s]))]  # by (label, caller index)
    labs = label[members]
    heads = np.flatnonzero(np.concatenate([[True], labs[1:] != labs[:-1]])) if len(members) \
        else np.zeros(0, dtype=np.int64)
    counts = np.diff(np.concatenate([heads, [len(members)]])).astype(np.int64)
    kept = np.flatnonzero(counts >= min_members)
    groups = np.zeros(len(kept), dtype=bh_amd.GROUP_DTYPE)
    for k, g in enumerate(kept):
        c = members[heads[g]:heads[g] + counts[g]]
        groups[k] = (labs[heads[g]], counts[g], heads[g], two_level(m[c]),
                     two_level(m[c] * x[c]), two_level(m[c] * y[c]), two_level(m[c] * vx[c]),
                     two_level(m[c] * vy[c]))
    if len(members) == 0:
        summary = (0, 0, 0, 0, -1, 0)
    else:
        big = int(np.argmax(counts))  # the first maximum: the lowest label
        summary = (n, len(members), len(heads), len(kept), int(labs[heads[big]]),
                   int(counts[big]))
    return dict(label=label, members=members.astype(np.int64), groups=groups, summary=summary)


def checker(arrs, cfg, link, min_members, fof=fof_all_pairs):
    """(catalogue, state after the build) for the bodies `arrs` through the oracle's tree."""
    idx, x, y, st, _ = candidates(arrs, cfg)
    label = labels_of(len(arrs[0]), idx, fof(idx, x, y, link))
    return catalogue(label, st, min_members), st


def chain(n=1000, seed=5):
    """n bodies at (600 + i, 300), mass 1, in a seeded random permutation of that order."""
    perm = np.random.default_rng(seed).permutation(n)
    x = 600.0 + perm.astype(np.float64)
    vel = np.random.default_rng(seed + 1).integers(-8, 9, (2, n)).astype(np.float64) / 4.0
    return x, np.full(n, 300.0), vel[0], vel[1], np.ones(n)


def spiral(n=4000, seed=7):
    """The chain wrapped into a square spiral of unit steps around (1200, 400) -- across the
    root cell's centre lines -- whose arms are 2 apart, in a seeded random permutation."""
    px, py = [0], [0]
    d, run = 0, 2
    while len(px) < n:
        for _ in range(2):
            for _ in range(run):
                px.append(px[-1] + (1, 0, -1, 0)[d])
                py.append(py[-1] + (0, 1, 0, -1)[d])
            d = (d + 1) % 4
        run += 2
    perm = np.random.default_rng(seed).permutation(n)
    x = 1200.0 + np.array(px[:n], dtype=np.float64)[perm]
    y = 400.0 + np.array(py[:n], dtype=np.float64)[perm]
    return x, y, np.zeros(n), np.zeros(n), np.ones(n)


# ---- checker self-tests ----------------------------------------------------------------------

CFG = make_cfg(theta=0.5)


@functools.lru_cache(maxsize=None)
def _two_disks():
    return candidates(scenes.two_disks(600, 200), CFG)


def _jitter_306():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "jitter_306.npz"))
    return candidates(tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z))[:3]


SMALL = {
    "jitter_306": _jitter_306,
    "spiral_1000": lambda: candidates(spiral(1000), CFG)[:3],
    "two_disks": lambda: _two_disks()[:3],
    "six_bodies": lambda: candidates(six_bodies(), CFG)[:3],
    "jitter_pair": lambda: candidates(jitter_pair(CFG), CFG)[:3],
    "chain": lambda: candidates(chain(), CFG)[:3],
}


@pytest.mark.parametrize("scene", sorted(SMALL))
def test_binned_equals_all_pairs(scene):
    idx, x, y = SMALL[scene]()
    for link in LINKS + (math.nextafter(1.0, 0.0), math.nextafter(20.0, 0.0)):
        assert np.array_equal(fof_binned(idx, x, y, link), fof_all_pairs(idx, x, y, link)), link


@pytest.mark.parametrize("scene", sorted(SMALL))
def test_both_equal_scipy(scene):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    idx, x, y = SMALL[scene]()
    for link in LINKS:
        adj = link_matrix(x, y, link)
        _, comp = csgraph.connected_components(sparse.csr_matrix(adj), directed=False)
        low = np.full(comp.max() + 1, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(low, comp, idx)
        assert np.array_equal(low[comp], fof_all_pairs(idx, x, y, link)), link
        assert np.array_equal(low[comp], fof_binned(idx, x, y, link)), link


@pytest.mark.parametrize("scene", sorted(SMALL))
def test_link_matrix_is_symmetric(scene):
    idx, x, y = SMALL[scene]()
    with np.errstate(all="ignore"):
        dx = x[:, None] - x[None, :]
        dy = y[:, None] - y[None, :]
        d2 = dx * dx + dy * dy
    same = dx == 0.0  # (equal coordinates: +0.0 against -0.0, the same square)
    assert np.array_equal(dx.view(np.int64)[~same], (-dx.T).view(np.int64)[~same])
    assert np.array_equal(same, same.T)
    assert np.array_equal(d2.view(np.int64), d2.T.view(np.int64))
    for link in LINKS:
        adj = link_matrix(x, y, link)
        assert np.array_equal(adj, adj.T) and adj.diagonal().all()


# groups (singletons included) and the largest group's size of two_disks(600, 200) per link
KNOWN = {0.0: (800, 1), 1.0: (771, 3), 4.0: (517, 34), 8.0: (308, 227), 20.0: (94, 448),
         50.0: (5, 793), math.inf: (1, 800)}


@pytest.mark.parametrize("link", LINKS)
def test_known_structures_of_the_default_tree(link):
    idx, x, y, st, _ = _two_disks()
    assert len(idx) == 800  # every body is in S
    cat = catalogue(labels_of(800, idx, fof_all_pairs(idx, x, y, link)), st, 1)
    assert (cat["summary"][2], cat["summary"][5]) == KNOWN[link]
    assert cat["summary"][:2] == (800, 800) and cat["summary"][3] == KNOWN[link][0]
    assert cat["groups"]["count"].sum() == 800 and len(cat["members"]) == 800


def test_catalogue_on_six_bodies():
    arrs = six_bodies()
    cat, st = checker(arrs, CFG, 20.0, 1)
    assert cat["label"].tolist() == [0, 1, 1, -1, -1, 5]  # 1-2 are 20 apart: `<=` links them
    assert cat["members"].tolist() == [0, 1, 2, 5]
    assert cat["groups"]["label"].tolist() == [0, 1, 5]
    assert cat["groups"]["first"].tolist() == [0, 1, 3]
    assert cat["groups"]["mass"].tolist() == [1.0, 5.0, -3.0]
    assert cat["groups"]["mx"].tolist() == [700.0, 2.0 * 1000.0 + 3.0 * 1020.0, -900.0]
    assert cat["summary"] == (6, 4, 3, 3, 1, 2)
    cat, _ = checker(arrs, CFG, math.nextafter(20.0, 0.0), 2)
    assert cat["label"].tolist() == [0, 1, 2, -1, -1, 5] and len(cat["groups"]) == 0
    assert cat["summary"] == (6, 4, 4, 0, 0, 1)  # all singletons: the lowest label is the largest
    empty = catalogue(np.full(3, -1, dtype=np.int64), tuple(np.zeros(3) for _ in range(5)), 1)
    assert empty["summary"] == (0, 0, 0, 0, -1, 0) and len(empty["members"]) == 0


def test_two_level_sum_order():
    """The sums are not numpy's pairwise ones: blocks of 256 in order, then the partials."""
    rng = np.random.default_rng(3)
    t = rng.uniform(-1.0, 1.0, 1000) * 10.0 ** rng.integers(-8, 9, 1000)
    want = 0.0
    for k in range(0, 1000, 256):
        part = 0.0
        for v in t[k:k + 256]:
            part = part + float(v)
        want = want + part
    assert two_level(t) == want
    assert math.copysign(1.0, two_level(np.array([-0.0]))) == 1.0  # from +0.0


def test_chain_and_spiral_shapes():
    for arrs, n in ((chain(), 1000), (spiral(), 4000)):
        idx, x, y, st, _ = candidates(arrs, CFG)
        assert len(idx) == n
        for a, b in zip(st, arrs):
            assert np.array_equal(a, b)  # exact coordinates, nothing jitters
        one = fof_binned(idx, x, y, 1.0)
        assert np.all(one == 0)  # one group, labelled by the list's first body
        assert np.array_equal(fof_binned(idx, x, y, math.nextafter(1.0, 0.0)), idx)
    x, y = spiral()[:2]
    assert x.min() < 1200.0 < x.max() and y.min() < 400.0 < y.max()  # across the centre lines


# ---- the ABI, without a GPU ------------------------------------------------------------------

def test_abi_symbols_and_struct_sizes():
    lib = bh_amd.load_library()
    for name in ("bh_find_groups", "bh_groups_kernel_ms"):
        assert hasattr(lib, name) and name in bh_amd.EXPORTED_SYMBOLS
    assert ctypes.sizeof(bh_amd.BhGroup) == 64 == bh_amd.GROUP_DTYPE.itemsize
    assert ctypes.sizeof(bh_amd.BhGroupsSummary) == 48
    assert [f[0] for f in bh_amd.BhGroup._fields_] == list(bh_amd.GROUP_DTYPE.names)


def test_null_handle_is_refused():
    lib = bh_amd.load_library()
    sm = bh_amd.BhGroupsSummary()
    assert lib.bh_find_groups(None, 1.0, 1, None, 0, None, 0, None, 0,
                              ctypes.byref(sm)) == bh_amd.BH_E_INVALID
    ms = ctypes.c_double(-7.0)
    assert lib.bh_groups_kernel_ms(None, ctypes.byref(ms)) == bh_amd.BH_E_INVALID
    assert ms.value == -7.0
