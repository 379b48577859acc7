"""CPU: the checker of bh_compute_radial_profile -- its definition in numpy -- with its own
properties on the ring scene, and the host-only part of the ABI (struct sizes, bh_radial_edges).

The checker states include/bh_engine.h's contract: elementwise separate binary64 operations, the
one special case R2 == 0, bins by a search of R itself in the edges (lower edge inclusive), the
members of a bin in ascending caller index, and strictly sequential sums in two levels -- blocks of
256 members from +0.0, then the block partials from +0.0.  tests/test_gpu_radial_profile.py
compares the device's bytes with it.
"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import bh_amd

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bh_engine.h")
TERMS = ("mass", "mr", "mvr", "mvt", "mvr2", "mvt2", "lz")
SUMMARY = ("n_bodies", "n_selected", "n_binned", "n_inner", "n_outer", "n_nan")
BLOCK = 256


def seq_sum(a):
    """The strictly sequential sum of a from +0.0 (np.sum would add pairwise)."""
    return np.cumsum(np.concatenate([np.zeros(1), np.asarray(a, dtype=np.float64)]))[-1]


def radial_terms(arrs, cx, cy, cvx, cvy):
    """(R, the seven term arrays) of every body."""
    x, y, vx, vy, m = (np.asarray(a, dtype=np.float64) for a in arrs)
    c = [np.float64(v) for v in (cx, cy, cvx, cvy)]
    with np.errstate(all="ignore"):
        dx = x - c[0]
        dy = y - c[1]
        R2 = dx * dx + dy * dy
        R = np.sqrt(R2)
        ux = vx - c[2]
        uy = vy - c[3]
        u = dx * ux + dy * uy
        w = dx * uy - dy * ux
        vr = np.where(R2 == 0.0, 0.0, u / R)
        vt = np.where(R2 == 0.0, 0.0, w / R)
        mvr = m * vr
        mvt = m * vt
        return R, [m, m * R, mvr, mvt, mvr * vr, mvt * vt, m * w]


def profile_ref(arrs, cx, cy, edges, cvx=0.0, cvy=0.0, subset=None):
    """(bins as a RADIAL_BIN_DTYPE array, the summary as a tuple in SUMMARY's order)."""
    edges = np.asarray(edges, dtype=np.float64)
    n_bin = len(edges) - 1
    N = len(arrs[0])
    R, terms = radial_terms(arrs, cx, cy, cvx, cvy)
    sel = np.ones(N, dtype=bool)
    if subset is not None:
        sel[:] = False
        sel[np.asarray(subset, dtype=np.int64)] = True
    nan = np.isnan(R)
    k = np.searchsorted(edges, np.where(nan, 0.0, R), side="right") - 1
    k[nan] = n_bin + 1  # set apart: in no bin
    bins = np.zeros(n_bin, dtype=bh_amd.RADIAL_BIN_DTYPE)
    for b in range(n_bin):
        mem = np.flatnonzero(sel & (k == b))  # ascending caller index
        bins["count"][b] = len(mem)
        for name, t in zip(TERMS, terms):
            partials = [seq_sum(t[mem[j:j + BLOCK]]) for j in range(0, len(mem), BLOCK)]
            bins[name][b] = seq_sum(partials)
    n_inner = int(np.sum(sel & ~nan & (k == -1)))
    n_outer = int(np.sum(sel & ~nan & (k == n_bin)))
    n_nan = int(np.sum(sel & nan))
    return bins, (N, int(sel.sum()), int(bins["count"].sum()), n_inner, n_outer, n_nan)


# ---- the ring scene ----------------------------------------------------------------------------

RING_CENTRE = (1200.0, 400.0)
RING_EDGES = np.arange(2.0, 17.0, 2.0)  # 2, 4, ..., 16: seven bins
RING_COUNTS = (1, 0, 255, 256, 257, 513, 2)  # the rings' bodies, bins 0..6
RING_BIN_COUNTS = (1, 0, 255, 256, 258, 513, 2)  # ... with the special at R = 10.0
RING_N = 1289


@functools.lru_cache(maxsize=None)
def ring_scene():
    """Rings of RING_COUNTS bodies inside the bins, five specials -- (1206, 408) at R = 10.0
    exactly, the centre itself, (1201, 400), a NaN x, (1300, 400) -- shuffled, with random
    velocities and masses in [0.5, 1.5).  Returns (x, y, vx, vy, m), the special's indices."""
    rng = np.random.default_rng(20261021)
    xs, ys = [], []
    for b, cnt in enumerate(RING_COUNTS):
        r = rng.uniform(RING_EDGES[b] + 0.125, RING_EDGES[b + 1] - 0.125, cnt)
        a = rng.uniform(0.0, 2.0 * math.pi, cnt)
        xs.append(RING_CENTRE[0] + r * np.cos(a))
        ys.append(RING_CENTRE[1] + r * np.sin(a))
    xs.append(np.array([1206.0, 1200.0, 1201.0, np.nan, 1300.0]))
    ys.append(np.array([408.0, 400.0, 400.0, 400.0, 400.0]))
    x, y = np.concatenate(xs), np.concatenate(ys)
    n = len(x)
    order = rng.permutation(n)
    x, y = x[order], y[order]
    where = np.empty(n, dtype=np.int64)
    where[order] = np.arange(n)
    vx, vy = rng.normal(0.0, 3.0, n), rng.normal(0.0, 3.0, n)
    m = rng.uniform(0.5, 1.5, n)
    for a in (x, y, vx, vy, m):
        a.setflags(write=False)
    return (x, y, vx, vy, m), tuple(int(i) for i in where[n - 5:])


def test_ring_scene_counts_are_the_constructed_ones():
    arrs, _ = ring_scene()
    assert len(arrs[0]) == RING_N
    bins, summary = profile_ref(arrs, *RING_CENTRE, RING_EDGES, 0.1, -0.2)
    assert tuple(bins["count"]) == RING_BIN_COUNTS
    assert summary == (RING_N, RING_N, 1285, 2, 1, 1)
    for name in TERMS:  # the empty bin is all zeros, +0.0
        assert bins[name][1].tobytes() == np.float64(0.0).tobytes()


def test_lower_edge_is_inclusive():
    arrs, special = ring_scene()
    at10 = special[0]
    R, _ = radial_terms(arrs, *RING_CENTRE, 0.0, 0.0)
    assert R[at10] == 10.0
    bins, _ = profile_ref(arrs, *RING_CENTRE, RING_EDGES, subset=[at10])
    assert RING_EDGES[4] == 10.0
    assert tuple(bins["count"]) == (0, 0, 0, 0, 1, 0, 0)
    assert bins["mr"][4] == arrs[4][at10] * 10.0


def test_classes_add_up_to_the_selection():
    arrs, _ = ring_scene()
    rng = np.random.default_rng(5)
    for subset in (None, rng.permutation(RING_N)[:RING_N // 2], [], np.arange(RING_N)):
        bins, s = profile_ref(arrs, *RING_CENTRE, RING_EDGES, subset=subset)
        assert s[2] == bins["count"].sum()
        assert s[2] + s[3] + s[4] + s[5] == s[1]
        assert s[1] == (RING_N if subset is None else len(subset))


def test_a_duplicate_counts_once():
    arrs, _ = ring_scene()
    half = np.random.default_rng(6).permutation(RING_N)[:600]
    twice = np.concatenate([half, half[::3], half[:5]])
    a, sa = profile_ref(arrs, *RING_CENTRE, RING_EDGES, subset=half)
    b, sb = profile_ref(arrs, *RING_CENTRE, RING_EDGES, subset=twice)
    assert a.tobytes() == b.tobytes() and sa == sb


def test_the_centre_body_has_no_direction():
    """R2 == 0: vr = vt = +0.0, so the body adds its mass and nothing else that could be NaN."""
    arrs, special = ring_scene()
    bins, s = profile_ref(arrs, *RING_CENTRE, [0.0, 1.0], 0.1, -0.2, subset=[special[1]])
    assert s == (RING_N, 1, 1, 0, 0, 0)
    m = arrs[4][special[1]]
    assert (bins["mass"][0], bins["mr"][0], bins["mvr"][0], bins["mvt"][0]) == (m, 0.0, 0.0, 0.0)
    assert not np.isnan(bins["lz"][0])


def test_two_levels_not_one():
    """A bin of more than 256 members is summed by blocks: it differs from one sequential sum
    somewhere on the ring scene (else the test scene could not tell the two rules apart)."""
    arrs, _ = ring_scene()
    bins, _ = profile_ref(arrs, *RING_CENTRE, [0.0, math.inf])
    _, terms = radial_terms(arrs, *RING_CENTRE, 0.0, 0.0)
    R, _ = radial_terms(arrs, *RING_CENTRE, 0.0, 0.0)
    mem = np.flatnonzero(~np.isnan(R))
    assert bins["count"][0] == len(mem) == RING_N - 1
    assert any(bins[name][0] != seq_sum(t[mem]) for name, t in zip(TERMS, terms))


# ---- the host-only ABI -------------------------------------------------------------------------

def test_struct_sizes_and_symbols():
    lib = bh_amd.load_library()
    assert ctypes.sizeof(bh_amd.BhRadialBin) == 64 == bh_amd.RADIAL_BIN_DTYPE.itemsize
    assert ctypes.sizeof(bh_amd.BhRadialSummary) == 48
    assert [f[0] for f in bh_amd.BhRadialBin._fields_] == list(bh_amd.RADIAL_BIN_DTYPE.names)
    assert [f[0] for f in bh_amd.BhRadialBin._fields_] == ["count"] + list(TERMS)
    assert [f[0] for f in bh_amd.BhRadialSummary._fields_] == list(SUMMARY)
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("bh_compute_radial_profile", "bh_radial_profile_kernel_ms", "bh_radial_edges"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(lib, name) and name in bh_amd.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+BH_RADIAL_MAX_BINS\s+4096\b", code)
    assert bh_amd.BH_RADIAL_MAX_BINS == 4096
    # the call is in the list of calls refused between bh_step_begin and bh_step_end
    assert "bh_compute_radial_profile" in txt[:txt.index("int bh_step_begin(")]
    for method in ("radial_profile", "radial_profile_kernel_ms"):
        assert callable(getattr(bh_amd.Engine, method))
    assert callable(bh_amd.PhysicsEngine.profile) and callable(bh_amd.radial_edges)


@pytest.mark.parametrize("n_bin", [1, 2, 7, 64, 4096])
@pytest.mark.parametrize("r", [(0.0, 1200.0), (0.1, 0.7), (3.0, 1e9)])
def test_linear_edges_are_the_formula(n_bin, r):
    r_min, r_max = r
    e = bh_amd.radial_edges(r_min, r_max, n_bin)
    want = np.array([r_min + (r_max - r_min) * (float(k) / float(n_bin)) for k in range(n_bin + 1)])
    want[0], want[-1] = r_min, r_max
    assert e.tobytes() == want.tobytes()
    assert e[0] == r_min and e[-1] == r_max and np.all(np.diff(e) > 0.0)


@pytest.mark.parametrize("n_bin", [1, 3, 64, 4096])
@pytest.mark.parametrize("r", [(1.0, 1024.0), (0.5, 1200.0), (1e-3, 1e6)])
def test_log_edges_increase_between_exact_ends(n_bin, r):
    r_min, r_max = r
    e = bh_amd.radial_edges(r_min, r_max, n_bin, log=True)
    assert len(e) == n_bin + 1 and e[0] == r_min and e[-1] == r_max
    assert np.all(np.diff(e) > 0.0)
    ratio = (r_max / r_min) ** (1.0 / n_bin)
    assert np.allclose(e[1:] / e[:-1], ratio, rtol=1e-9, atol=0.0)
    if r == (1.0, 1024.0) and n_bin == 1:
        assert e.tolist() == [1.0, 1024.0]


def _edges_rc(r_min, r_max, n_bin, log, null=False):
    lib = bh_amd.load_library()
    out = np.full(max(n_bin, 0) + 1 if n_bin <= 4096 else 1, -7.0)
    rc = lib.bh_radial_edges(float(r_min), float(r_max), int(n_bin), int(log),
                             None if null else out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return rc, out, lib.bh_last_error(None).decode()


@pytest.mark.parametrize("case", [
    dict(r_min=0.0, r_max=1.0, n_bin=4, log=0, null=True),
    dict(r_min=0.0, r_max=1.0, n_bin=0, log=0),
    dict(r_min=0.0, r_max=1.0, n_bin=-1, log=0),
    dict(r_min=0.0, r_max=1.0, n_bin=4097, log=0),
    dict(r_min=-1.0, r_max=1.0, n_bin=4, log=0),
    dict(r_min=math.nan, r_max=1.0, n_bin=4, log=0),
    dict(r_min=math.inf, r_max=math.inf, n_bin=4, log=0),
    dict(r_min=1.0, r_max=1.0, n_bin=4, log=0),
    dict(r_min=2.0, r_max=1.0, n_bin=4, log=0),
    dict(r_min=1.0, r_max=math.nan, n_bin=4, log=0),
    dict(r_min=1.0, r_max=math.inf, n_bin=4, log=0),
    dict(r_min=0.0, r_max=1.0, n_bin=4, log=1),          # log spacing needs r_min > 0
    dict(r_min=1.0, r_max=1.0 + 2.0 ** -50, n_bin=64, log=0),   # not strictly increasing
    dict(r_min=1.0, r_max=1.0 + 2.0 ** -50, n_bin=64, log=1),
])
def test_edges_refusals(case):
    rc, out, err = _edges_rc(**case)
    assert rc == bh_amd.BH_E_INVALID
    assert "bh_radial_edges" in err
    assert np.all(out == -7.0)  # nothing written
    rc, _, _ = _edges_rc(1.0, 2.0, 4, 0)
    assert rc == bh_amd.BH_OK


def test_radial_profile_formulas():
    """RadialProfile's derived read-outs are their documented formulas; an empty bin gives NaN,
    not an exception."""
    arrs, _ = ring_scene()
    bins, s = profile_ref(arrs, *RING_CENTRE, RING_EDGES, 0.1, -0.2)
    p = bh_amd.RadialProfile(RING_EDGES, bins, bh_amd.RadialSummary(*s))
    e = RING_EDGES
    with np.errstate(all="ignore"):
        mass = bins["mass"]
        want = dict(surface_density=mass / (np.pi * (e[1:] ** 2 - e[:-1] ** 2)),
                    v_rot=bins["mvt"] / mass, v_rad=bins["mvr"] / mass,
                    sigma_r=np.sqrt(bins["mvr2"] / mass - (bins["mvr"] / mass) ** 2),
                    sigma_t=np.sqrt(bins["mvt2"] / mass - (bins["mvt"] / mass) ** 2),
                    mean_r=bins["mr"] / mass, enclosed_mass=np.cumsum(mass))
    for name, w in want.items():
        assert np.array_equal(getattr(p, name), w, equal_nan=True), name
    for name in ("v_rot", "v_rad", "sigma_r", "sigma_t", "mean_r"):
        got = getattr(p, name)
        assert np.isnan(got[1]) and not np.isnan(np.delete(got, 1)).any(), name
    assert p.surface_density[1] == 0.0 and p.summary.n_binned == 1285
    assert np.array_equal(p.count, RING_BIN_COUNTS) and p.mass.tobytes() == mass.tobytes()
    assert np.all(np.abs(p.mean_r - 0.5 * (e[1:] + e[:-1]))[[0, 2, 3, 4, 5, 6]] < 1.0)
