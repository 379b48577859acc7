"""GPU: bh_compute_radial_profile / bh_radial_profile_kernel_ms / Engine.radial_profile /
PhysicsEngine.profile.

Every comparison is on the bytes of `bins` and `summary` against the checker of
tests/test_radial_profile_ref.py -- the definition in numpy -- fed with get_bodies() of the same
engine after the call.  The calls go through the raw ABI so that every output can be given or
withheld, with sentinels around the arrays.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from conftest import bits_equal
from test_potential_ref import cfg_from_golden, make_cfg, params_of
from test_radial_profile_ref import (RING_BIN_COUNTS, RING_CENTRE, RING_EDGES, RING_N, SUMMARY,
                                     profile_ref, ring_scene)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("x", "y", "vx", "vy", "m")
_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)
SENTINEL = -77
PAD = 2  # sentinel records in front of and behind the bins
CFG = make_cfg(theta=0.5)
CENTRE = (1200.0, 400.0)


def _engine(arrs, cfg=CFG, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    return eng


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    return tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z)


def call(eng, cx, cy, edges, cvx=0.0, cvy=0.0, subset=None, bins=True, summary=True,
         n_bin=None, n_subset=None, null_edges=False):
    """(rc, bins or None, summary tuple or None) of one raw call; the guard records around the
    outputs must still hold the sentinel afterwards."""
    e = np.ascontiguousarray(edges, dtype=np.float64)
    n_bin = len(e) - 1 if n_bin is None else n_bin
    room = max(n_bin, 0) if n_bin <= bh_amd.BH_RADIAL_MAX_BINS else 0
    buf = np.full((room + 2 * PAD) * 8, SENTINEL, dtype=np.int64)
    sm = np.full(6 + 2 * PAD, SENTINEL, dtype=np.int64)
    sub = None
    if subset is not None:  # (one spare entry: an empty subset still has a pointer)
        sub = np.concatenate([np.asarray(subset, dtype=np.int64).reshape(-1),
                              np.zeros(1, dtype=np.int64)])
        n_subset = len(sub) - 1 if n_subset is None else n_subset
    bp = ctypes.cast(buf.ctypes.data + 64 * PAD, ctypes.POINTER(bh_amd.BhRadialBin))
    sp = ctypes.cast(sm.ctypes.data + 8 * PAD, ctypes.POINTER(bh_amd.BhRadialSummary))
    rc = eng._lib.bh_compute_radial_profile(
        eng._h, float(cx), float(cy), float(cvx), float(cvy), int(n_bin),
        None if null_edges else e.ctypes.data_as(_D),
        None if sub is None else sub.ctypes.data_as(_I64P), n_subset or 0,
        bp if bins else None, sp if summary else None)
    rec = buf.reshape(-1, 8)
    assert np.all(rec[:PAD] == SENTINEL) and np.all(rec[PAD + room:] == SENTINEL), "bins guards"
    assert np.all(sm[:PAD] == SENTINEL) and np.all(sm[PAD + 6:] == SENTINEL), "summary guards"
    if rc != bh_amd.BH_OK or not bins:
        assert np.all(rec == SENTINEL), "bins written by a call that was not to write them"
    if rc != bh_amd.BH_OK or not summary:
        assert np.all(sm == SENTINEL), "summary written by a call that was not to write it"
    got_bins = rec[PAD:PAD + room].copy().view(bh_amd.RADIAL_BIN_DTYPE).reshape(-1) \
        if bins and rc == bh_amd.BH_OK else None
    got_sum = tuple(int(v) for v in sm[PAD:PAD + 6]) if summary and rc == bh_amd.BH_OK else None
    return rc, got_bins, got_sum


def err(eng):
    return eng._lib.bh_last_error(eng._h).decode()


def _one_nan(bins):
    """bins with every NaN replaced by one NaN."""
    out = bins.copy()
    for f in bh_amd.RADIAL_BIN_DTYPE.names[1:]:
        out[f][np.isnan(out[f])] = np.nan
    return out


def check(eng, cx, cy, edges, cvx=0.0, cvy=0.0, subset=None, what="", made_nans=False):
    """One call against the checker on get_bodies() after it; returns (bins, summary).
    made_nans: the inputs make the arithmetic produce NaNs of its own (inf - inf, 0 * inf).  IEEE
    754 leaves the sign of such a NaN open, and the host's multiplier and the device's choose
    differently (0 * -inf: sign bit set on the host, clear on the MI355X), so there a NaN must
    meet a NaN and every other value is still compared by its bytes."""
    rc, bins, summary = call(eng, cx, cy, edges, cvx, cvy, subset)
    assert rc == bh_amd.BH_OK, err(eng)
    want_bins, want_sum = profile_ref(eng.get_bodies(), cx, cy, edges, cvx, cvy, subset)
    if made_nans:
        bins, want_bins = _one_nan(bins), _one_nan(want_bins)
    assert summary == want_sum, f"{what}summary {dict(zip(SUMMARY, summary))}"
    assert np.array_equal(bins["count"], want_bins["count"]), f"{what}count"
    for f in bh_amd.RADIAL_BIN_DTYPE.names[1:]:
        assert np.array_equal(bins[f].view(np.int64), want_bins[f].view(np.int64)), f"{what}{f}"
    assert bins.tobytes() == want_bins.tobytes(), what
    return bins, summary


# ---- 1. the ring scene -------------------------------------------------------------------------

def _ring_subsets():
    rng = np.random.default_rng(11)
    half = rng.permutation(RING_N)[:RING_N // 2]
    return dict(none=None, half=half, empty=np.zeros(0, dtype=np.int64), all=np.arange(RING_N),
                duplicates=np.concatenate([half, half[::2], half[:7]]))


@pytest.mark.parametrize("state", ["fresh", "after a build"])
def test_ring_scene(state):
    arrs, _ = ring_scene()
    eng = _engine(arrs)
    if state == "after a build":  # slot order is no longer caller order
        eng.compute_accelerations()
    results = {}
    for name, subset in _ring_subsets().items():
        results[name] = check(eng, *RING_CENTRE, RING_EDGES, 0.1, -0.2, subset, what=f"{name}: ")
    if state == "fresh":
        assert tuple(results["none"][0]["count"]) == RING_BIN_COUNTS
        assert results["none"][1] == (RING_N, RING_N, 1285, 2, 1, 1)
    assert results["all"][0].tobytes() == results["none"][0].tobytes()
    assert results["duplicates"][0].tobytes() == results["half"][0].tobytes()
    assert results["duplicates"][1] == results["half"][1]
    assert results["empty"][1][1:] == (0, 0, 0, 0, 0)
    assert results["empty"][0].tobytes() == bytes(64 * 7)
    eng.close()


# ---- 2. caller order after removals, and the caller-visible state ------------------------------

@pytest.mark.parametrize("name,calls", [("merge_127.npz", (4, 2)), ("jitter_306.npz", (1,))])
def test_after_steps(name, calls):
    arrs, cfg = _golden(name)
    eng = _engine(arrs, cfg)
    for k in calls:
        eng.step(k)
    if name.startswith("merge"):
        assert eng.num_bodies() < len(arrs[0])
    x, y = eng.get_bodies()[:2]
    centre = (float(np.median(x)), float(np.median(y)))
    r_max = float(np.max(np.hypot(x - centre[0], y - centre[1]))) * 0.75
    for edges in ([0.0, math.inf], bh_amd.radial_edges(0.0, r_max, 16)):
        bins, summary = check(eng, *centre, edges, what=f"{len(edges) - 1} bins: ")
        assert summary[2] > 0
    eng.close()


# ---- 3. block edges at the second level --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _uniform():
    return scenes.uniform(70_000, 0.5)


@pytest.mark.parametrize("edges", ["one bin", "4096 bins"])
def test_many_blocks_and_many_bins(edges):
    eng = _engine(_uniform())
    e = [0.0, math.inf] if edges == "one bin" else bh_amd.radial_edges(0.0, 2600.0, 4096)
    bins, summary = check(eng, *CENTRE, e)
    assert summary[2] == 70_000
    if edges == "one bin":
        assert bins["count"][0] == 70_000 > 256 * 256  # more than 256 partials for one lane
    else:
        assert np.count_nonzero(bins["count"] == 0) > 0 and bins["count"].max() < 256
    eng.close()


# ---- 4. two disks, a group's members in the group's own frame ----------------------------------

def test_two_disks_and_a_group():
    eng = _engine(scenes.two_disks(600, 200))
    eng.step(3)
    check(eng, *CENTRE, bh_amd.radial_edges(0.0, 400.0, 64), what="linear: ")
    check(eng, *CENTRE, bh_amd.radial_edges(1.0, 400.0, 64, log=True), what="log: ")
    _, _, cat, mem = eng.find_groups(30.0, 20, labels=False, members=True)
    assert len(cat) >= 1
    g = cat[int(np.argmax(cat["count"]))]
    members = mem[int(g["first"]):int(g["first"] + g["count"])]
    centre = (g["mx"] / g["mass"], g["my"] / g["mass"])
    frame = (g["px"] / g["mass"], g["py"] / g["mass"])
    bins, summary = check(eng, *centre, bh_amd.radial_edges(0.0, 320.0, 64), *frame,
                          subset=members, what="group: ")
    assert summary[1] == g["count"] and summary[2] > 0
    eng.close()


# ---- 5. odd inputs -----------------------------------------------------------------------------

def test_odd_inputs():
    x, y, vx, vy, m = (a.copy() for a in scenes.two_disks(300, 100))
    x[7] = 1e300          # outer, even with a last edge of +inf
    m[11] = 0.0           # counted
    m[13] = -2.5          # counted
    eng = _engine((x, y, vx, vy, m))
    bins, summary = check(eng, *CENTRE, [0.0, math.inf], what="+inf edge: ")
    assert summary == (400, 400, 399, 0, 1, 0) and bins["count"][0] == 399
    check(eng, *CENTRE, bh_amd.radial_edges(0.0, 350.0, 16), what="16 bins: ")
    bins, summary = check(eng, *CENTRE, [0.0, math.inf], subset=[11, 13], what="m <= 0: ")
    assert bins["count"][0] == 2 and bins["mass"][0] == -2.5
    _, summary = check(eng, math.nan, 400.0, [0.0, 10.0, math.inf], what="NaN centre: ")
    assert summary == (400, 400, 0, 0, 0, 400)
    bins, _ = check(eng, *CENTRE, bh_amd.radial_edges(0.0, 350.0, 8), math.inf, 0.0,
                    what="inf cvx: ", made_nans=True)
    assert np.isnan(bins["lz"][:7]).all() and not np.isnan(bins["mass"]).any()
    _, summary = check(eng, *CENTRE, [25.0, 50.0, 100.0], what="edges[0] > 0: ")
    assert summary[3] > 0 and summary[4] > 0
    eng.close()


def test_bodies_outside_the_root_are_in():
    arrs, cfg = _golden("outside_153.npz")
    eng = _engine(arrs, cfg)
    eng.step(1)
    bins, summary = check(eng, *CENTRE, [0.0, math.inf])
    assert summary[2] == eng.num_bodies() == bins["count"][0]
    x, y = eng.get_bodies()[:2]
    root_h = max(cfg["width_px"], cfg["height_px"]) / 2.0 + 2.0
    out = (np.abs(x - cfg["width_px"] / 2.0) >= root_h) | (np.abs(y - cfg["height_px"] / 2.0) >= root_h)
    assert out.any()
    check(eng, *CENTRE, bh_amd.radial_edges(0.0, 4000.0, 16), subset=np.flatnonzero(out))
    eng.close()


# ---- 6. output combinations, refusals and empty cases ------------------------------------------

def test_output_combinations():
    arrs, _ = ring_scene()
    eng = _engine(arrs)
    rc, full_bins, full_sum = call(eng, *RING_CENTRE, RING_EDGES, 0.1, -0.2)
    assert rc == bh_amd.BH_OK
    for bins in (False, True):
        for summary in (False, True):
            rc, b, s = call(eng, *RING_CENTRE, RING_EDGES, 0.1, -0.2, bins=bins, summary=summary)
            assert rc == bh_amd.BH_OK
            assert (b is not None, s is not None) == (bins, summary)
            if bins:
                assert b.tobytes() == full_bins.tobytes()
            if summary:
                assert s == full_sum
    eng.close()


def test_refusals():
    arrs, _ = ring_scene()
    eng = _engine(arrs)
    before = eng.radial_profile_kernel_ms()
    N = RING_N
    nan = math.nan
    cases = [
        (dict(edges=RING_EDGES, null_edges=True), "edges is NULL"),
        (dict(edges=[1.0], n_bin=0), "n_bin"),
        (dict(edges=[1.0], n_bin=-3), "n_bin"),
        (dict(edges=np.arange(4098.0), n_bin=4097), "n_bin"),
        (dict(edges=[0.0, nan, 2.0]), "NaN"),
        (dict(edges=[0.0, 1.0, nan]), "NaN"),
        (dict(edges=[-1.0, 1.0, 2.0]), "edges[0]"),
        (dict(edges=[0.0, 1.0, 1.0]), "strictly increasing"),
        (dict(edges=[0.0, 2.0, 1.0]), "strictly increasing"),
        (dict(edges=[0.0, math.inf, math.inf]), "strictly increasing"),
        (dict(edges=RING_EDGES, subset=[0, 1], n_subset=-1), "n_subset"),
        (dict(edges=RING_EDGES, subset=[0, 1], n_subset=(1 << 28) + 1), "n_subset"),
        (dict(edges=RING_EDGES, subset=[0, -1, 2]), "subset index"),
        (dict(edges=RING_EDGES, subset=[0, N, 2]), "subset index"),
    ]
    for kw, text in cases:
        rc, _, _ = call(eng, *RING_CENTRE, **kw)
        assert rc == bh_amd.BH_E_INVALID, kw
        assert "bh_compute_radial_profile" in err(eng) and text in err(eng), (kw, err(eng))
    assert eng._lib.bh_compute_radial_profile(None, 0.0, 0.0, 0.0, 0.0, 1, None, None, 0, None,
                                              None) == bh_amd.BH_E_INVALID
    assert eng.radial_profile_kernel_ms() == before == 0.0  # nothing was launched
    rc, _, s = call(eng, *RING_CENTRE, [0.0, 1.0, math.inf], subset=[N - 1, 0])  # legal
    assert rc == bh_amd.BH_OK and s[1] == 2
    eng.close()


def test_async_guard():
    eng = _engine(scenes.two_disks(300, 100))
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        rc, _, _ = call(eng, *CENTRE, [0.0, 100.0])
        assert rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    check(eng, *CENTRE, [0.0, 100.0])
    eng.close()


def test_no_bodies():
    eng = bh_amd.Engine(params_of(CFG), device=0)
    z = np.zeros(0)
    for _ in range(2):
        rc, bins, summary = call(eng, *CENTRE, RING_EDGES, subset=None)
        assert rc == bh_amd.BH_OK
        assert bins.tobytes() == bytes(64 * 7) and summary == (0,) * 6
        rc, bins, summary = call(eng, *CENTRE, RING_EDGES, subset=[])
        assert rc == bh_amd.BH_OK and summary == (0,) * 6
        rc, _, _ = call(eng, *CENTRE, RING_EDGES, subset=[0])
        assert rc == bh_amd.BH_E_INVALID  # no index is inside [0, 0)
        eng.reset_bodies(z, z, z, z, z)
    eng.close()


# ---- 7. the state is untouched -----------------------------------------------------------------

def test_state_untouched():
    arrs = scenes.two_disks(1500, 500)
    a, b = _engine(arrs), _engine(arrs)
    a.step(2)
    b.step(2)
    edges = bh_amd.radial_edges(0.0, 400.0, 32)
    check(a, *CENTRE, edges)
    check(a, *CENTRE, edges, subset=np.arange(0, 1000, 3))
    for name, u, v in zip(FIELDS, a.get_bodies(), b.get_bodies()):
        assert bits_equal(u, v), f"{name} after the calls"
    for u, v in zip(a.get_quads(), b.get_quads()):
        assert bits_equal(u, v), "quads after the calls"
    call(a, *CENTRE, edges)  # (and once more on the tree get_quads left)
    a.step(2)
    b.step(2)  # (no profile on this engine before its steps)
    for name, u, v in zip(FIELDS, a.get_bodies(), b.get_bodies()):
        assert bits_equal(u, v), f"{name} two steps after the calls"
    a.close()
    b.close()


# ---- 8. the same bytes -------------------------------------------------------------------------

def test_deterministic_and_multi_handle(monkeypatch):
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    arrs = scenes.two_disks(1500, 500)
    one = _engine(arrs)
    one.step(3)
    edges = bh_amd.radial_edges(0.0, 400.0, 64)
    half = np.arange(0, one.num_bodies(), 2)
    first = [check(one, *CENTRE, edges, 1.0, 2.0), check(one, *CENTRE, edges, 1.0, 2.0, half)]
    fresh = _engine(one.get_bodies())
    two = _engine(one.get_bodies(), devices=[0, 0])
    assert two.multi_world() == 2
    for eng, what in ((one, "second call"), (fresh, "fresh engine"), (two, "multi handle"),
                      (two, "its second call")):
        for subset, want in zip((None, half), first):
            rc, bins, summary = call(eng, *CENTRE, edges, 1.0, 2.0, subset)
            assert rc == bh_amd.BH_OK, err(eng)
            assert bins.tobytes() == want[0].tobytes() and summary == want[1], what
    assert two.radial_profile_kernel_ms() > 0.0
    for eng in (one, fresh, two):
        eng.close()


# ---- 9. the stopwatch --------------------------------------------------------------------------

def test_stopwatch():
    eng = _engine(scenes.two_disks(300, 100))
    assert eng.radial_profile_kernel_ms() == 0.0
    call(eng, *CENTRE, [0.0, 100.0], bins=False, summary=False)  # validates, launches nothing
    assert eng.radial_profile_kernel_ms() == 0.0
    check(eng, *CENTRE, [0.0, 100.0])
    ms = eng.radial_profile_kernel_ms()
    assert ms > 0.0
    z = np.zeros(0)
    eng.reset_bodies(z, z, z, z, z)
    rc, _, summary = call(eng, *CENTRE, [0.0, 100.0])
    assert rc == bh_amd.BH_OK and summary == (0,) * 6
    assert eng.radial_profile_kernel_ms() == ms  # left as it was
    eng.close()


# ---- 10. the Python surfaces -------------------------------------------------------------------

def test_engine_radial_profile_and_derived_arrays():
    eng = _engine(scenes.two_disks(600, 200))
    eng.step(2)
    edges = bh_amd.radial_edges(0.0, 400.0, 24)
    subset = np.arange(0, 600)
    p = eng.radial_profile(*CENTRE, edges, cvx=0.5, cvy=-0.5, subset=subset)
    want_bins, want_sum = profile_ref(eng.get_bodies(), *CENTRE, edges, 0.5, -0.5, subset)
    assert p.bins.tobytes() == want_bins.tobytes()
    assert tuple(getattr(p.summary, f) for f in SUMMARY) == want_sum
    assert np.array_equal(p.edges, edges)
    with np.errstate(all="ignore"):
        mass = want_bins["mass"]
        want = dict(surface_density=mass / (np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)),
                    v_rot=want_bins["mvt"] / mass, v_rad=want_bins["mvr"] / mass,
                    sigma_r=np.sqrt(want_bins["mvr2"] / mass - (want_bins["mvr"] / mass) ** 2),
                    sigma_t=np.sqrt(want_bins["mvt2"] / mass - (want_bins["mvt"] / mass) ** 2),
                    mean_r=want_bins["mr"] / mass, enclosed_mass=np.cumsum(mass))
    for name, w in want.items():
        assert np.array_equal(getattr(p, name), w, equal_nan=True), name
    assert (p.count == 0).any() and np.isnan(p.v_rot[p.count == 0]).all()  # no exception
    # a disk that rotates: |v_rot| well above the dispersions where the bins are populated
    busy = p.count >= 20
    assert busy.any() and np.median(np.abs(p.v_rot[busy])) > 3.0 * np.nanmedian(p.sigma_t[busy])
    assert eng.radial_profile(*CENTRE, edges, subset=[]).summary.n_selected == 0
    eng.close()


def test_physics_engine_profile():
    x, y, vx, vy, m = scenes.two_disks(600, 200)
    bodies = [bh_amd.Body(*(float(a[i]) for a in (x, y, vx, vy, m))) for i in range(len(x))]
    pe = bh_amd.PhysicsEngine(bodies)
    pe.step()
    edges = bh_amd.radial_edges(0.0, 300.0, 12)
    galaxies = pe.groups(30.0, 50)
    assert len(galaxies) >= 1
    galaxy = max(galaxies, key=len)
    idx = [i for i, b in enumerate(bodies) if any(b is g for g in galaxy)]
    assert len(idx) == len(galaxy)
    arrs = tuple(np.array([getattr(b, f) for b in bodies]) for f in FIELDS)
    for chosen, subset in ((None, None), (galaxy, idx), (galaxy[::-1] + galaxy[:3], idx), ([], [])):
        p = pe.profile(*CENTRE, edges, vx=0.25, vy=0.0, bodies=chosen)
        want_bins, want_sum = profile_ref(arrs, *CENTRE, edges, 0.25, 0.0, subset)
        assert p.bins.tobytes() == want_bins.tobytes()
        assert tuple(getattr(p.summary, f) for f in SUMMARY) == want_sum
    bodies[5].x += 1.0  # an edit of the caller's list is pushed first, as pick and nearest do
    arrs = tuple(np.array([getattr(b, f) for b in bodies]) for f in FIELDS)
    p = pe.profile(*CENTRE, edges)
    assert p.bins.tobytes() == profile_ref(arrs, *CENTRE, edges)[0].tobytes()
    with pytest.raises(ValueError):
        pe.profile(*CENTRE, edges, bodies=[bh_amd.Body(0.0, 0.0, 0.0, 0.0, 1.0)])
