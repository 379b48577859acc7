"""GPU: bh_find_knn / bh_find_knn_bodies / bh_knn_kernel_ms / PhysicsEngine.nearest.

Every value is compared exactly (d2 as its int64 view) with the checker of tests/test_knn_ref.py:
the candidate set from the oracle's tree of the same start state, the definition applied to it
with numpy on the positions the build left -- which are asserted to be eng.get_bodies() after the
call.  The calls go through the raw ABI so that every output can be given or withheld.  A scene
whose build jitters bodies gets a fresh engine for every call: every call builds, and jitters.
"""
import ctypes
import functools
import itertools
import math
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from test_field_ref import make_probes, root_cell
from test_knn_ref import knn_brute
from test_neighbors_ref import FIELDS, candidates, jitter_pair, six_bodies
from test_potential_ref import cfg_from_golden, make_cfg, params_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)
OUTPUTS = ("idx", "d2", "found")
SENTINEL = -77
CFG = make_cfg(theta=0.5)
# both sides of every change of bh_knn_shape's waves per workgroup (10|11, 21|22, 42|43)
KS = (1, 2, 7, 8, 10, 11, 21, 22, 42, 43, 64)
RS = (0.0, 0.5, 8.0, math.inf)


def _engine(arrs, cfg, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    return eng


def _dp(a):
    return a.ctypes.data_as(_D) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(_I64P) if a is not None else None


def _outputs(n, k, want, extra=0):
    """Sentinel-filled arrays for the outputs in `want` (None for the others), with `extra`
    entries of room past what the call may write."""
    return dict(idx=np.full(n * k + extra, SENTINEL, dtype=np.int64) if "idx" in want else None,
                d2=np.full(n * k + extra, -7.0) if "d2" in want else None,
                found=np.full(n + extra, SENTINEL, dtype=np.int64) if "found" in want else None)


def knn(eng, px, py, k, r_max, want=OUTPUTS, extra=0):
    """(rc, outputs) of one raw bh_find_knn call."""
    px = np.ascontiguousarray(px, dtype=np.float64)
    py = np.ascontiguousarray(py, dtype=np.float64)
    out = _outputs(len(px), k, want, extra)
    rc = eng._lib.bh_find_knn(eng._h, len(px), _dp(px), _dp(py), k, float(r_max), _ip(out["idx"]),
                              _dp(out["d2"]), _ip(out["found"]))
    return rc, out


def knn_bodies(eng, k, r_max, want=OUTPUTS, rows_cap=None, extra=0):
    """(rc, outputs, n_rows) of one raw bh_find_knn_bodies call with room for rows_cap rows."""
    cap = eng.num_bodies() if rows_cap is None else rows_cap
    out = _outputs(cap, k, want, extra)
    rows = ctypes.c_int64(SENTINEL)
    rc = eng._lib.bh_find_knn_bodies(eng._h, k, float(r_max), _ip(out["idx"]), _dp(out["d2"]),
                                     _ip(out["found"]), cap, ctypes.byref(rows))
    return rc, out, rows.value


def assert_rows(got, want, n, k, what=""):
    """The outputs `got` holds equal the checker's (idx[n, k], d2[n, k], found[n]) -- or another
    call's dict -- and nothing past them was written."""
    if isinstance(want, dict):
        want = tuple(None if want[o] is None else want[o][:m] for o, m in
                     zip(OUTPUTS, (n * k, n * k, n)))
    wi, wd, wf = (None if w is None else np.asarray(w).ravel() for w in want)
    if got["idx"] is not None and wi is not None:
        assert np.array_equal(got["idx"][:n * k], wi), f"{what}idx"
        assert np.all(got["idx"][n * k:] == SENTINEL), f"{what}idx past the rows"
    if got["d2"] is not None and wd is not None:
        assert np.array_equal(got["d2"][:n * k].view(np.int64), wd.view(np.int64)), f"{what}d2"
        assert np.all(got["d2"][n * k:] == -7.0), f"{what}d2 past the rows"
    if got["found"] is not None and wf is not None:
        assert np.array_equal(got["found"][:n], wf), f"{what}found"
        assert np.all(got["found"][n:] == SENTINEL), f"{what}found past the rows"


def assert_state(eng, st, what=""):
    for name, a, b in zip(FIELDS, eng.get_bodies(), st):
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"{what}{name}"


def check(arrs, cfg, cand, px, py, k, r_max, eng=None):
    """One bh_find_knn call on a fresh engine (or `eng`) against the checker."""
    own = eng is None
    eng = eng or _engine(arrs, cfg)
    idx, x, y, st, _ = cand
    rc, got = knn(eng, px, py, k, r_max, extra=3)
    assert rc == bh_amd.BH_OK, eng._lib.bh_last_error(eng._h)
    assert_rows(got, knn_brute(idx, x, y, px, py, k, r_max), len(px), k, f"k={k} r={r_max}: ")
    assert_state(eng, st)
    if own:
        eng.close()
    return got


def check_bodies(arrs, cfg, cand, k, r_max, eng=None):
    """One bh_find_knn_bodies call on a fresh engine (or `eng`) against the checker's self mode."""
    own = eng is None
    eng = eng or _engine(arrs, cfg)
    idx, x, y, st, _ = cand
    n = len(st[0])
    rc, got, rows = knn_bodies(eng, k, r_max, extra=3)
    assert rc == bh_amd.BH_OK, eng._lib.bh_last_error(eng._h)
    assert rows == n
    want = knn_brute(idx, x, y, st[0], st[1], k, r_max, own=np.arange(n, dtype=np.int64))
    assert_rows(got, want, n, k, f"bodies k={k} r={r_max}: ")
    assert not (got["idx"][:n * k].reshape(n, k) == np.arange(n)[:, None]).any()  # never itself
    assert_state(eng, st)
    if own:
        eng.close()
    return got


# ---- the scenes, their candidates and probes, made once ---------------------------------------

def _golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    return tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(arrs, cfg, candidates, px, py): 120 probes in make_probes' mix plus 20 on bodies where the
    build left them."""
    if name == "two_disks":
        arrs, cfg = scenes.two_disks(600, 200), CFG
    elif name == "jitter_pair":
        arrs, cfg = jitter_pair(CFG), CFG
    else:
        arrs, cfg = _golden(name + ".npz")
    cand = candidates(arrs, cfg)
    px, py = make_probes(arrs, cfg, 120, 23)
    st = cand[3]
    on = np.random.default_rng(29).choice(len(st[0]), min(20, len(st[0])), replace=False)
    return arrs, cfg, cand, np.concatenate([px, st[0][on]]), np.concatenate([py, st[1][on]])


def test_two_disks_every_k_and_radius():
    arrs, cfg, cand, px, py = _scene("two_disks")
    eng = _engine(arrs, cfg)
    full = 0
    for k, r in itertools.product(KS, RS):
        got = check(arrs, cfg, cand, px, py, k, r, eng=eng)
        full += int((got["found"][:len(px)] == k).sum())
        if r == 0.0:  # the probes on bodies find them, with d2 = 0
            assert np.all(got["found"][120:140] >= 1)
            assert np.all(got["d2"][:len(px) * k].reshape(-1, k)[120:, 0] == 0.0)
        if r == math.inf:
            assert np.all(got["found"][:len(px)] == k)
    assert full > 0
    for k, r in ((1, math.inf), (8, 8.0), (11, math.inf), (43, 0.5), (64, math.inf)):
        check_bodies(arrs, cfg, cand, k, r, eng=eng)
    eng.close()


@pytest.mark.parametrize("name", ["jitter_306", "outside_153", "jitter_pair"])
def test_scenes(name):
    arrs, cfg, cand, px, py = _scene(name)
    for k, r in ((1, math.inf), (8, math.inf), (11, math.inf), (43, math.inf), (64, math.inf),
                 (8, 0.0), (8, 0.5), (8, 8.0)):
        check(arrs, cfg, cand, px, py, k, r)
    # the bodies as probes: those not in S (outside the root, dropped by the jitter, mass 0) too
    assert len(cand[0]) < len(arrs[0])
    for k, r in ((1, math.inf), (8, math.inf), (22, 8.0), (64, math.inf)):
        check_bodies(arrs, cfg, cand, k, r)


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    cx, cy, h = root_cell(CFG)
    x = rng.uniform(cx - 0.9 * h, cx + 0.9 * h, n)
    y = rng.uniform(cy - 0.9 * h, cy + 0.9 * h, n)
    return x, y, np.zeros(n), np.zeros(n), np.ones(n)


@pytest.mark.parametrize("n", [6, 63, 64, 65, 70])
def test_k_around_the_size_of_S(n):
    """k = |S| - 1, |S|, |S| + 1 on six_bodies; k = 64 on 63, 64, 65 and 70 bodies, where it
    (nearly) empties S -- for the probes and, one body fewer, for the bodies themselves."""
    arrs = six_bodies() if n == 6 else _uniform(n, 100 + n)
    cand = candidates(arrs, CFG)
    size = len(cand[0])
    assert size == (4 if n == 6 else n)
    px, py = make_probes(arrs, CFG, 40, 7)
    px, py = np.concatenate([px, arrs[0]]), np.concatenate([py, arrs[1]])
    eng = _engine(arrs, CFG)
    for k in ((3, 4, 5) if n == 6 else (63, 64)):
        got = check(arrs, CFG, cand, px, py, k, math.inf, eng=eng)
        assert np.all(got["found"][:len(px)] == min(k, size))
        check_bodies(arrs, CFG, cand, k, math.inf, eng=eng)
    eng.close()


# ---- probe counts: every change of the launch shape -------------------------------------------

def _shape_counts():
    """1, 63, 64, 65, both sides of every change of bh_knn_shape's lanes per wave up to 8192, and
    the first count whose workgroups hold several waves and whose last one is partial."""
    counts = {1, 63, 64, 65}
    prev = bh_amd.knn_shape(1, 8)[0]
    for n in range(2, 8193):
        cur = bh_amd.knn_shape(n, 8)[0]
        if cur != prev:
            counts |= {n - 1, n}
        prev = cur
    lo, hi = 8192, 1 << 20
    assert bh_amd.knn_shape(lo, 8)[1] == 1 < bh_amd.knn_shape(hi, 8)[1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if bh_amd.knn_shape(mid, 8)[1] == 1 else (lo, mid)
    n = hi
    while _last_group_waves(n, 8) in (0, 1):
        n += 1
    return sorted(counts | {n})


def _last_group_waves(n, k):
    bpw, wpb, _, _ = bh_amd.knn_shape(n, k)
    return (-(-n // bpw)) % wpb


SHAPE_COUNTS = _shape_counts()
K_MANY = 22  # the reference is made once at k = 22; a row's first k entries are the row for k


@functools.lru_cache(maxsize=None)
def _small_tree():
    arrs = scenes.two_disks(90, 30)
    return arrs, candidates(arrs, CFG)


@functools.lru_cache(maxsize=None)
def _probes_many():
    arrs, _ = _small_tree()
    # (lists of 4096, one seed each: the mix draws its on-body probes without replacement)
    parts = [make_probes(arrs, CFG, 4096, 31 + j) for j in range(-(-SHAPE_COUNTS[-1] // 4096))]
    return tuple(np.concatenate(p)[:SHAPE_COUNTS[-1]] for p in zip(*parts))


@functools.lru_cache(maxsize=None)
def _want_many():
    idx, x, y, _, _ = _small_tree()[1]
    return knn_brute(idx, x, y, *_probes_many(), K_MANY, 60.0)


def _cut(want, n, k):
    """The checker's rows for the first n probes and the first k entries of each."""
    return want[0][:n, :k], want[1][:n, :k], np.minimum(want[2][:n], k)


def test_shape_counts_cover_every_workgroup_size():
    n = SHAPE_COUNTS[-1]
    assert {1, 63, 64, 65} <= set(SHAPE_COUNTS) and len(SHAPE_COUNTS) >= 8
    assert [bh_amd.knn_shape(n, k)[1] for k in (8, 11, 22)] == [8, 4, 2]
    assert all(_last_group_waves(n, k) > 1 for k in (8, 11))  # partial last workgroups
    assert _want_many()[2].min() < 8 < K_MANY <= _want_many()[2].max()  # short rows and full ones


@pytest.mark.parametrize("n", SHAPE_COUNTS)
def test_probe_counts(n):
    px, py = _probes_many()
    arrs, _ = _small_tree()
    eng = _engine(arrs, CFG)
    for k in ((8,) if n < SHAPE_COUNTS[-1] else (8, 11, K_MANY)):  # 8, 4 and 2 waves per group
        rc, got = knn(eng, px[:n], py[:n], k, 60.0, extra=3)
        assert rc == bh_amd.BH_OK
        assert_rows(got, _cut(_want_many(), n, k), n, k, f"k={k}: ")
    eng.close()


# ---- ties, odd inputs -------------------------------------------------------------------------

def test_lattice_ties():
    """6 x 6 equal bodies 10 apart: probes on lattice points and cell centres have many equal
    d2, and the lower index wins at every rank."""
    gx, gy = np.meshgrid(500.0 + 10.0 * np.arange(6), 300.0 + 10.0 * np.arange(6))
    arrs = (gx.ravel(), gy.ravel(), np.zeros(36), np.zeros(36), np.ones(36))
    cand = candidates(arrs, CFG)
    assert len(cand[0]) == 36
    inner = (arrs[0] < 550.0) & (arrs[1] < 350.0)  # the 25 cells' lower left corners
    px = np.concatenate([arrs[0], arrs[0][inner] + 5.0])
    py = np.concatenate([arrs[1], arrs[1][inner] + 5.0])
    eng = _engine(arrs, CFG)
    for k in (1, 2, 4, 5, 9, 36, 37):
        got = check(arrs, CFG, cand, px, py, k, math.inf, eng=eng)
        check(arrs, CFG, cand, px, py, k, 10.0, eng=eng)
        check_bodies(arrs, CFG, cand, k, math.inf, eng=eng)
    d2 = got["d2"][:len(px) * 37].reshape(-1, 37)
    assert np.all(d2[36:, :4] == 50.0) and np.all(d2[:36, 0] == 0.0)  # the ties are there
    eng.close()


def test_three_coincident_bodies():
    x, y, vx, vy, m = six_bodies()
    arrs = (np.concatenate([x, [900.0] * 3]), np.concatenate([y, [450.0] * 3]), np.zeros(9),
            np.zeros(9), np.concatenate([m, [1.0, 2.0, 3.0]]))
    cand = candidates(arrs, CFG)
    st = cand[3]
    px = np.concatenate([[900.0, 900.0, 899.0], st[0][6:], arrs[0][:3]])
    py = np.concatenate([[450.0, 450.5, 450.0], st[1][6:], arrs[1][:3]])
    for k in (1, 2, 3, 4, 8):
        check(arrs, CFG, cand, px, py, k, math.inf)
        check(arrs, CFG, cand, px, py, k, 2e-3)
        check_bodies(arrs, CFG, cand, k, math.inf)


def test_odd_probes():
    arrs, cfg, cand, _, _ = _scene("outside_153")
    cx, cy, h = root_cell(cfg)
    px = np.array([cx + 3 * h, cx - 2 * h, 2.0 ** 40, 1e300, -1e300, math.nan, cx, math.nan, cx,
                   math.inf, cx])
    py = np.array([cy, cy + 5 * h, 2.0 ** 40, 1e300, cy, cy, math.nan, math.nan, cy, cy,
                   -math.inf])
    for k in (1, 5, 64):
        got = check(arrs, cfg, cand, px, py, k, math.inf)
        rows_i = got["idx"][:len(px) * k].reshape(-1, k)
        rows_d = got["d2"][:len(px) * k].reshape(-1, k)
        assert np.all(got["found"][[5, 6, 7]] == 0) and np.all(rows_i[[5, 6, 7]] == -1)
        # at 1e300 every d2 is +inf: the row is the k lowest indices of S
        for j in (3, 4, 9, 10):
            assert np.all(np.isinf(rows_d[j])) and rows_i[j].tolist() == cand[0][:k].tolist()
        check(arrs, cfg, cand, px, py, k, 1e300)
        check(arrs, cfg, cand, px, py, k, 3 * h)


def _dozen():
    """test_gpu_neighbors' twelve: six_bodies; 6 and 7, both of negative mass, alone in a cell, so
    the internal node above them has mass 0 and hides them; 8 of negative mass beside 9 of
    positive mass (found); 10 of mass 0 beside 11."""
    x, y, vx, vy, m = six_bodies()
    x = np.concatenate([x, [2000.0, 2000.5, 1800.0, 1800.5, 400.0, 400.5]])
    y = np.concatenate([y, [700.0, 700.5, 100.0, 100.5, 100.0, 100.5]])
    m = np.concatenate([m, [-1.0, -2.0, -4.0, 5.0, 0.0, 6.0]])
    return x, y, np.zeros(12), np.zeros(12), m


def test_zero_and_negative_masses():
    arrs = _dozen()
    cand = candidates(arrs, CFG)
    assert cand[0].tolist() == [0, 1, 2, 5, 8, 9, 11]  # 6 and 7 lie under a mass-0 internal node
    px = np.concatenate([arrs[0], arrs[0] + 0.25, [1200.0]])
    py = np.concatenate([arrs[1], arrs[1] + 0.25, [400.0]])
    eng = _engine(arrs, CFG)
    for k, r in itertools.product((1, 3, 6, 7, 8), (0.0, 1.0, 400.0, math.inf)):
        got = check(arrs, CFG, cand, px, py, k, r, eng=eng)
        assert not np.isin(got["idx"][:len(px) * k], [3, 4, 6, 7, 10]).any()
        check_bodies(arrs, CFG, cand, k, r, eng=eng)
    eng.close()


def test_seed_independence():
    """Probes at both ends of the Morton curve (the root cell's first and last corner) with all
    bodies in the opposite corner: whatever window the seed took, the result is the checker's."""
    cx, cy, h = root_cell(CFG)
    rng = np.random.default_rng(3)
    ends = ((cx - h + 1e-6, cy - h + 1e-6), (cx + h - 1e-6, cy + h - 1e-6))
    for (ax, ay), (bx, by) in (ends, ends[::-1]):
        x = ax + np.sign(cx - ax) * rng.uniform(0.0, 60.0, 200)  # the bodies near corner a
        y = ay + np.sign(cy - ay) * rng.uniform(0.0, 60.0, 200)
        arrs = (x, y, np.zeros(200), np.zeros(200), np.ones(200))
        cand = candidates(arrs, CFG)
        assert len(cand[0]) == 200
        px = np.array([bx, ax, bx, cx, 2 * bx - cx])  # the far corner, the near one, between, beyond
        py = np.array([by, ay, ay, cy, 2 * by - cy])
        eng = _engine(arrs, CFG)
        for k in (1, 8, 64):
            check(arrs, CFG, cand, px, py, k, math.inf, eng=eng)
            check(arrs, CFG, cand, px, py, k, 2.5 * h, eng=eng)
            check_bodies(arrs, CFG, cand, k, math.inf, eng=eng)
        eng.close()


# ---- outputs, capacity, the contract ----------------------------------------------------------

def test_null_outputs():
    arrs, cfg, cand, px, py = _scene("two_disks")
    n, k = len(px), 8
    eng = _engine(arrs, cfg)
    rc, full = knn(eng, px, py, k, 8.0)
    assert rc == bh_amd.BH_OK
    rc, full_b, rows = knn_bodies(eng, k, 8.0)
    assert rc == bh_amd.BH_OK and rows == len(arrs[0])
    for m in range(len(OUTPUTS) + 1):
        for want in itertools.combinations(OUTPUTS, m):
            rc, part = knn(eng, px, py, k, 8.0, want=want, extra=5)
            assert rc == bh_amd.BH_OK, want
            assert all((part[o] is None) == (o not in want) for o in OUTPUTS)
            assert_rows(part, full, n, k, f"{want}: ")
            rc, part, rows = knn_bodies(eng, k, 8.0, want=want, extra=5)
            assert rc == bh_amd.BH_OK and rows == len(arrs[0]), want
            assert_rows(part, full_b, rows, k, f"bodies {want}: ")
    eng.close()


def test_rows_cap():
    arrs, cfg, cand, _, _ = _scene("two_disks")
    n = len(arrs[0])
    eng = _engine(arrs, cfg)
    for cap in (n - 1, 0):
        rc, got, rows = knn_bodies(eng, 5, math.inf, rows_cap=cap, extra=7)
        assert rc == bh_amd.BH_E_CAPACITY and rows == n
        assert b"bh_find_knn_bodies" in eng._lib.bh_last_error(eng._h)
        assert np.all(got["idx"] == SENTINEL) and np.all(got["d2"] == -7.0)  # untouched
        assert np.all(got["found"] == SENTINEL)
    assert_state(eng, cand[3])  # the build still happened
    check_bodies(arrs, cfg, cand, 5, math.inf, eng=eng)  # the re-call with room
    rc, got, rows = knn_bodies(eng, 5, math.inf, rows_cap=n + 9)
    assert rc == bh_amd.BH_OK and rows == n
    # n_rows is nullable
    out = _outputs(n, 5, OUTPUTS)
    assert eng._lib.bh_find_knn_bodies(eng._h, 5, math.inf, _ip(out["idx"]), _dp(out["d2"]),
                                       _ip(out["found"]), n, None) == bh_amd.BH_OK
    assert_rows(out, got, n, 5)
    # the Python mirror
    idx, x, y, st, _ = cand
    want = knn_brute(idx, x, y, st[0], st[1], 5, math.inf, own=np.arange(n))
    pi, pd, pf = eng.find_knn_bodies(5)
    assert pi.shape == pd.shape == (n, 5) and pf.shape == (n,)
    assert np.array_equal(pi, want[0]) and np.array_equal(pd, want[1]) \
        and np.array_equal(pf, want[2])
    eng.close()


def test_no_probes_and_no_bodies():
    arrs, cfg, cand, _, _ = _scene("two_disks")
    eng = _engine(arrs, cfg)
    rc, got = knn(eng, np.zeros(0), np.zeros(0), 4, 1.0, extra=4)
    assert rc == bh_amd.BH_OK
    assert_rows(got, (np.zeros((0, 4)), np.zeros((0, 4)), np.zeros(0)), 0, 4)
    assert_state(eng, cand[3])  # the build still happened
    assert eng._lib.bh_find_knn(eng._h, 0, None, None, 4, 1.0, None, None, None) == bh_amd.BH_OK
    eng.close()
    empty = tuple(np.zeros(0) for _ in range(5))
    eng = _engine(empty, CFG)
    px, py = np.array([1200.0, 3.0, math.nan]), np.array([400.0, 4.0, 1.0])
    rc, got = knn(eng, px, py, 3, math.inf)
    assert rc == bh_amd.BH_OK
    assert np.all(got["found"] == 0) and np.all(got["idx"] == -1) and np.all(np.isinf(got["d2"]))
    rc, got, rows = knn_bodies(eng, 3, math.inf, rows_cap=0, extra=2)
    assert rc == bh_amd.BH_OK and rows == 0
    assert np.all(got["idx"] == SENTINEL) and np.all(got["found"] == SENTINEL)
    i, d, f = eng.find_knn_bodies(3)
    assert i.shape == d.shape == (0, 3) and f.shape == (0,)
    eng.close()


def _refusals():
    one = np.array([1000.0])
    d = one.ctypes.data_as(_D)

    def call(lib, h, n=1, px=d, py=d, k=4, r=1.0):
        return lib.bh_find_knn(h, n, px, py, k, r, None, None, None)

    def bodies(lib, h, k=4, r=1.0, cap=100):
        return lib.bh_find_knn_bodies(h, k, r, None, None, None, cap, None)
    count = "bh_find_knn: n_probe must be in [0, 2^28]"
    return [("negative", lambda lib, h: call(lib, h, n=-1), count, one),
            ("too-many", lambda lib, h: call(lib, h, n=(1 << 28) + 1), count, one),
            ("px-null", lambda lib, h: call(lib, h, px=None), "bh_find_knn: px or py is NULL", one),
            ("py-null", lambda lib, h: call(lib, h, py=None), "bh_find_knn: px or py is NULL", one),
            ("k-zero", lambda lib, h: call(lib, h, k=0), "bh_find_knn: k must be in 1..64", one),
            ("k-65", lambda lib, h: call(lib, h, k=65), "bh_find_knn: k must be in 1..64", one),
            ("k-zero-no-probes", lambda lib, h: call(lib, h, n=0, k=0),
             "bh_find_knn: k must be in 1..64", one),
            ("r-nan", lambda lib, h: call(lib, h, r=math.nan), "bh_find_knn: r_max must be >= 0",
             one),
            ("r-negative", lambda lib, h: call(lib, h, r=-1.0), "bh_find_knn: r_max must be >= 0",
             one),
            ("batches", lambda lib, h: call(lib, h, n=1 << 28, k=8),
             "bh_find_knn: more than 2^31 - 1 entries in all: ask in batches", one),
            ("bodies-k", lambda lib, h: bodies(lib, h, k=65),
             "bh_find_knn_bodies: k must be in 1..64", one),
            ("bodies-r", lambda lib, h: bodies(lib, h, r=-0.5),
             "bh_find_knn_bodies: r_max must be >= 0", one),
            ("bodies-r-nan", lambda lib, h: bodies(lib, h, r=math.nan),
             "bh_find_knn_bodies: r_max must be >= 0", one),
            ("bodies-cap", lambda lib, h: bodies(lib, h, cap=-1),
             "bh_find_knn_bodies: rows_cap must be >= 0", one)]


_REFUSALS = _refusals()


@pytest.mark.parametrize("call,text", [r[1:3] for r in _REFUSALS], ids=[r[0] for r in _REFUSALS])
def test_refusal(call, text):
    arrs = six_bodies()
    eng = _engine(arrs, CFG)
    assert call(eng._lib, eng._h) == bh_amd.BH_E_INVALID
    assert eng._lib.bh_last_error(eng._h).decode() == text
    assert_state(eng, arrs)  # refused before anything was built
    assert eng.knn_kernel_ms() == 0.0  # ... or launched
    eng.close()


def test_null_handle():
    lib = bh_amd.load_library()
    one = np.array([1000.0])
    d = one.ctypes.data_as(_D)
    assert lib.bh_find_knn(None, 1, d, d, 1, 1.0, None, None, None) == bh_amd.BH_E_INVALID
    assert lib.bh_find_knn_bodies(None, 1, 1.0, None, None, None, 0, None) == bh_amd.BH_E_INVALID


def test_async_guard():
    eng = _engine(scenes.two_disks(300, 100), CFG)
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        assert knn(eng, [1.0], [2.0], 3, 5.0)[0] == bh_amd.BH_E_STATE
        assert knn_bodies(eng, 3, 5.0, rows_cap=400)[0] == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    rc, got = knn(eng, [1.0], [2.0], 3, 5.0)
    assert rc == bh_amd.BH_OK and got["found"].tolist() == [0]
    eng.close()


@pytest.mark.parametrize("bodies", [False, True])
def test_state_semantics_of_compute_accelerations(bodies):
    arrs, cfg = _golden("jitter_306.npz")
    px, py = make_probes(arrs, cfg, 100, 43)
    a, b = _engine(arrs, cfg), _engine(arrs, cfg)
    rc = knn_bodies(a, 8, math.inf)[0] if bodies else knn(a, px, py, 8, math.inf)[0]
    assert rc == bh_amd.BH_OK
    b.compute_accelerations()
    assert_state(a, b.get_bodies(), "after the call: ")
    a.step(2)
    b.step(2)
    assert_state(a, b.get_bodies(), "after step(2): ")
    a.close()
    b.close()


def test_deterministic_and_multi_handle(monkeypatch):
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    arrs, cfg, cand, px, py = _scene("two_disks")
    n, nb, k = len(px), len(arrs[0]), 8
    one = _engine(arrs, cfg)
    two = _engine(arrs, cfg, devices=[0, 0])
    assert two.multi_world() == 2
    rc, first = knn(one, px, py, k, 50.0)
    assert rc == bh_amd.BH_OK
    rc, first_b, _ = knn_bodies(one, k, 50.0)
    assert rc == bh_amd.BH_OK
    for eng, what in ((one, "second call: "), (two, "multi handle: "), (two, "its second: ")):
        rc, again = knn(eng, px, py, k, 50.0)
        assert rc == bh_amd.BH_OK
        assert_rows(again, first, n, k, what)
        rc, again, rows = knn_bodies(eng, k, 50.0)
        assert rc == bh_amd.BH_OK and rows == nb
        assert_rows(again, first_b, nb, k, what + "bodies: ")
    assert_state(two, one.get_bodies())
    one.step(2)
    two.step(2)
    assert_state(two, one.get_bodies(), "after step(2): ")
    assert two.knn_kernel_ms() > 0.0
    two.close()
    one.close()


def _ms(eng):
    ms = ctypes.c_double(-7.0)
    return eng._lib.bh_knn_kernel_ms(eng._h, ctypes.byref(ms)), ms.value


def test_stopwatch():
    eng = _engine(six_bodies(), CFG)
    fn = eng._lib.bh_knn_kernel_ms
    assert fn(eng._h, None) == bh_amd.BH_E_INVALID
    assert fn(None, ctypes.byref(ctypes.c_double(0.0))) == bh_amd.BH_E_INVALID
    assert _ms(eng) == (bh_amd.BH_OK, 0.0)  # nothing launched yet: exactly 0.0
    assert knn(eng, np.zeros(0), np.zeros(0), 2, 1.0)[0] == bh_amd.BH_OK
    assert _ms(eng) == (bh_amd.BH_OK, 0.0), "a call without a launch started the watch"
    assert knn(eng, [700.0], [300.0], 2, 1.0)[0] == bh_amd.BH_OK
    rc, first = _ms(eng)
    assert rc == bh_amd.BH_OK and math.isfinite(first) and first > 0.0, (rc, first)
    assert knn(eng, np.zeros(0), np.zeros(0), 2, 1.0)[0] == bh_amd.BH_OK
    assert _ms(eng) == (bh_amd.BH_OK, first), "a call without a launch moved the watch"
    assert eng.knn_kernel_ms() == first
    assert knn_bodies(eng, 2, math.inf)[0] == bh_amd.BH_OK
    assert eng.knn_kernel_ms() > 0.0
    eng.close()


def test_python_find_knn_and_the_radius_lists():
    """Engine.find_knn's rows equal find_neighbors' lists at r = r_max, sorted by (d2, index)
    and cut at k."""
    arrs, cfg, cand, px, py = _scene("two_disks")
    k, r = 6, 12.0
    eng = _engine(arrs, cfg)
    gi, gd, gf = eng.find_knn(px, py, k, r)
    assert gi.shape == gd.shape == (len(px), k) and gf.shape == (len(px),)
    _, _, _, offsets, indices = eng.find_neighbors(px, py, r, lists=True)
    x, y = eng.get_bodies()[:2]
    assert 0 < gf.min() < k == gf.max() or gf.min() == 0
    for j in range(len(px)):
        ids = indices[offsets[j]:offsets[j + 1]]
        dx, dy = x[ids] - px[j], y[ids] - py[j]
        d2 = dx * dx + dy * dy
        order = np.lexsort((ids, d2))[:k]
        assert gf[j] == len(order)
        assert gi[j, :gf[j]].tolist() == ids[order].tolist() and np.all(gi[j, gf[j]:] == -1)
        assert np.array_equal(gd[j, :gf[j]], d2[order]) and np.all(np.isinf(gd[j, gf[j]:]))
    gi2, gd2, gf2 = eng.find_knn(px, py, k)  # r_max defaults to +inf
    assert np.all(gf2 == k) and np.array_equal(gi2[gf == k], gi[gf == k])
    with pytest.raises(bh_amd.BhError):
        eng.find_knn(px, py, 65)
    eng.close()


def test_nearest_returns_the_callers_bodies():
    arrs = _dozen()
    bodies = [bh_amd.Body(*(float(a[i]) for a in arrs)) for i in range(12)]
    pe = bh_amd.PhysicsEngine(bodies)
    idx, x, y, _, _ = candidates(arrs, make_cfg())
    for qx, qy, k, r in ((1010.0, 300.0, 2, 10.0), (1010.0, 300.0, 3, 9.0),
                         (2000.2, 700.2, 4, 5.0), (1800.2, 100.2, 2, 5.0),
                         (400.0, 100.0, 3, 1.0), (5000.0, 300.0, 1, 50.0),
                         (699.0, 301.0, 64, math.inf), (699.0, 301.0, 5, math.inf)):
        wi, _, wf = knn_brute(idx, x, y, [qx], [qy], k, r)
        got = pe.nearest(qx, qy, k, r)
        assert len(got) == wf[0], (qx, qy, k, r)
        assert all(g is bodies[int(c)] for g, c in zip(got, wi[0])), (qx, qy, k, r)
    assert [b is c for b, c in zip(pe.nearest(1010.0, 300.0, 2), bodies[1:3])] == [True, True]
    assert pe.nearest(2000.2, 700.2, 4, 5.0) == []      # hidden under a mass-0 node
    assert len(pe.nearest(0.0, 0.0, 64)) == 7            # all of S, no more
    assert pe.get_bodies() is bodies and len(bodies) == 12
