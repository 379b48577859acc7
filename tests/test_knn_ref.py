"""The checker of the k-nearest query (bh_find_knn, bh_find_knn_bodies) and its launch shape, on CPU.

`knn_brute(...)` applies the query's definition to test_neighbors_ref.candidates()' set with
numpy: d2 = dx*dx + dy*dy in separate IEEE operations, the mask d2 <= r_max*r_max, np.lexsort by
(caller index, d2), cut at k, pad with -1 and +inf.  No tree pruning, no seed and no heap is
restated here.  tests/test_gpu_knn.py compares the engine exactly against it.

bh_knn_shape is host-only, so its properties are checked here too.
"""
import ctypes
import math

import numpy as np
import pytest

import bh_amd
from test_neighbors_ref import brute, candidates, six_bodies
from test_potential_ref import make_cfg

_I64P = ctypes.POINTER(ctypes.c_int64)


def knn_brute(idx, x, y, px, py, k, r_max, own=None):
    """(idx[n, k], d2[n, k], found[n]) of the definition on the candidates (idx, x, y).  own:
    per probe the caller index that is no candidate of it (bh_find_knn_bodies), or None."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    n, m = len(px), len(idx)
    out_i = np.full((n, k), -1, dtype=np.int64)
    out_d = np.full((n, k), np.inf)
    found = np.zeros(n, dtype=np.int64)
    r_max = np.float64(r_max)
    if m == 0:
        return out_i, out_d, found
    with np.errstate(all="ignore"):
        for lo in range(0, n, 2048):  # probes x candidates, a block at a time
            rows = slice(lo, min(lo + 2048, n))
            dx = x[None, :] - px[rows, None]
            dy = y[None, :] - py[rows, None]
            d2 = dx * dx + dy * dy
            hit = (r_max >= 0) & (d2 <= r_max * r_max)
            if own is not None:
                hit &= idx[None, :] != np.asarray(own)[rows, None]
            ids = np.broadcast_to(idx, d2.shape)
            order = np.lexsort((ids, d2, ~hit), axis=-1)[:, :k]  # the hits first, by (d2, index)
            cnt = np.minimum(hit.sum(axis=1), k)
            keep = np.arange(order.shape[1])[None, :] < cnt[:, None]
            w = order.shape[1]
            out_i[rows, :w] = np.where(keep, np.take_along_axis(ids, order, axis=1), -1)
            out_d[rows, :w] = np.where(keep, np.take_along_axis(d2, order, axis=1), np.inf)
            found[rows] = cnt
    return out_i, out_d, found


def knn_checker(arrs, cfg, px, py, k, r_max):
    """(knn_brute's rows, state after the build) for probes (px, py) on the bodies `arrs`."""
    idx, x, y, st, _ = candidates(arrs, cfg)
    return knn_brute(idx, x, y, px, py, k, r_max), st


def knn_bodies_checker(arrs, cfg, k, r_max):
    """The same with the bodies themselves as probes, each without its own body."""
    idx, x, y, st, _ = candidates(arrs, cfg)
    own = np.arange(len(st[0]), dtype=np.int64)
    return knn_brute(idx, x, y, st[0], st[1], k, r_max, own=own), st


def from_lists(idx, x, y, px, py, k, r):
    """The rows made from the radius query's lists (brute): sorted by (d2, index) and cut at k."""
    got = brute(idx, x, y, px, py, r)
    pos = {int(c): i for i, c in enumerate(idx)}
    n = len(px)
    out_i = np.full((n, k), -1, dtype=np.int64)
    out_d = np.full((n, k), np.inf)
    found = np.zeros(n, dtype=np.int64)
    for j in range(n):
        ids = got["indices"][got["offsets"][j]:got["offsets"][j + 1]]
        at = np.array([pos[int(c)] for c in ids], dtype=np.int64)
        with np.errstate(all="ignore"):
            dx, dy = x[at] - px[j], y[at] - py[j]
            d2 = dx * dx + dy * dy
        order = np.lexsort((ids, d2))[:k]
        found[j] = len(order)
        out_i[j, :len(order)] = ids[order]
        out_d[j, :len(order)] = d2[order]
    return out_i, out_d, found


def test_checker_on_six_bodies():
    arrs = six_bodies()
    cfg = make_cfg()
    idx, x, y, st, _ = candidates(arrs, cfg)
    assert idx.tolist() == [0, 1, 2, 5]
    # the tie at (1010, 300) goes to index 1, then 2
    gi, gd, gf = knn_brute(idx, x, y, [1010.0], [300.0], 2, math.inf)
    assert gi.tolist() == [[1, 2]] and gd.tolist() == [[100.0, 100.0]] and gf.tolist() == [2]
    gi, gd, gf = knn_brute(idx, x, y, [1010.0], [300.0], 1, math.inf)
    assert gi.tolist() == [[1]] and gf.tolist() == [1]
    # a probe on body 0 finds it first, with d2 = 0
    gi, gd, gf = knn_brute(idx, x, y, [700.0], [300.0], 3, math.inf)
    assert gi[0, 0] == 0 and gd[0, 0] == 0.0 and gf.tolist() == [3]
    assert np.all(np.diff(gd[0]) >= 0)
    # out-of-root (3) and mass-0 (4) bodies are never found, not by a probe on them; the
    # negative-mass body (5) is
    gi, gd, gf = knn_brute(idx, x, y, arrs[0], arrs[1], 6, math.inf)
    assert not np.isin(gi, [3, 4]).any() and np.all(gf == 4)
    assert gi[5, 0] == 5 and gd[5, 0] == 0.0
    # k beyond |S| pads with -1 and +inf
    assert np.all(gi[:, 4:] == -1) and np.all(np.isinf(gd[:, 4:]))
    assert np.all(np.sort(gi[:, :4], axis=1) == [0, 1, 2, 5])
    # the cap: r_max = 10 at the tie finds both, just below it nothing; r_max = 0 the coincident
    assert knn_brute(idx, x, y, [1010.0], [300.0], 4, 10.0)[2].tolist() == [2]
    gi, gd, gf = knn_brute(idx, x, y, [1010.0], [300.0], 4, math.nextafter(10.0, 0.0))
    assert gf.tolist() == [0] and gi.tolist() == [[-1] * 4] and np.all(np.isinf(gd))
    assert knn_brute(idx, x, y, [700.0], [300.0], 4, 0.0)[0].tolist() == [[0, -1, -1, -1]]
    # a NaN coordinate finds nothing; a probe at 1e300 finds all at d2 = +inf, ordered by index
    gi, gd, gf = knn_brute(idx, x, y, [math.nan, 1e300], [0.0, 1e300], 3, math.inf)
    assert gf.tolist() == [0, 3] and gi[1].tolist() == [0, 1, 2] and np.all(np.isinf(gd[1]))
    # self mode drops exactly the own body
    (si, sd, sf), _ = knn_bodies_checker(arrs, cfg, 4, math.inf)
    for i in range(6):
        want = [c for c in (0, 1, 2, 5) if c != i]
        assert sorted(si[i, :sf[i]].tolist()) == want and i not in si[i]
    assert sf.tolist() == [3, 3, 3, 4, 4, 3]
    assert si[1, 0] == 2 and sd[1, 0] == 400.0


@pytest.mark.parametrize("k,r", [(1, 8.0), (3, 50.0), (8, math.inf), (64, 400.0)])
def test_equals_the_radius_lists_sorted_and_cut(k, r):
    from bh_amd import scenes
    cfg = make_cfg(theta=0.5)
    idx, x, y, st, _ = candidates(scenes.two_disks(90, 30), cfg)
    rng = np.random.default_rng(5)
    px = np.concatenate([rng.uniform(0.0, cfg["width_px"], 40), st[0][:10]])
    py = np.concatenate([rng.uniform(0.0, cfg["height_px"], 40), st[1][:10]])
    a = knn_brute(idx, x, y, px, py, k, r)
    b = from_lists(idx, x, y, px, py, k, r)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
    assert a[2].max() == min(k, len(idx)) or r < math.inf


SHAPE_LANES = (0, 1, 63, 64, 65, 1000, 8192, 65535, 65536, 100000, 524287, 524288, 1 << 20, 1 << 28)


def test_knn_shape_fits_the_budget():
    seen = set()
    for n in SHAPE_LANES:
        bpw0, wpb0, _ = bh_amd.tracer_launch_shape(n)  # walk_shape's choices for n lanes
        for k in range(1, 65):
            bpw, wpb, lds, grid = bh_amd.knn_shape(n, k)
            assert bpw == bpw0 and 1 <= wpb <= wpb0
            assert lds == wpb * 64 * k * 12 <= 65536
            # halved no further than needed
            assert wpb == wpb0 or 2 * wpb * 64 * k * 12 > 65536
            assert grid == -(-(-(-n // bpw)) // wpb)
            seen.add(wpb)
    assert seen == {1, 2, 4, 8}
    # 8 waves up to k = 10, 1 wave from k = 43
    assert [bh_amd.knn_shape(100000, k)[1] for k in (1, 10, 11, 21, 22, 42, 43, 64)] == \
        [8, 8, 4, 4, 2, 2, 1, 1]


def test_knn_shape_refusals():
    lib = bh_amd.load_library()
    out = np.full(4, -7, dtype=np.int64)
    o = out.ctypes.data_as(_I64P)
    assert lib.bh_knn_shape(100, 8, None) == bh_amd.BH_E_INVALID
    for n, k in ((-1, 8), ((1 << 28) + 1, 8), (100, 0), (100, 65), (100, -1)):
        assert lib.bh_knn_shape(n, k, o) == bh_amd.BH_E_INVALID, (n, k)
    assert np.all(out == -7)
    assert lib.bh_knn_shape(1 << 28, 64, o) == bh_amd.BH_OK and out[1] == 1
    with pytest.raises(bh_amd.BhError):
        bh_amd.knn_shape(10, 65)
