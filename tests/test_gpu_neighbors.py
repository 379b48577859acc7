"""GPU: bh_find_neighbors / bh_neighbors_kernel_ms / PhysicsEngine.pick.

Every value is compared exactly with the checker of tests/test_neighbors_ref.py: the candidate
set from the oracle's tree of the same start state, the query's definition applied to it with
numpy on the positions the build left -- which are asserted to be eng.get_bodies() after the call.
The calls go through the raw ABI so that every output can be given or withheld.
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
from test_neighbors_ref import FIELDS, brute, candidates, jitter_pair, six_bodies
from test_potential_ref import cfg_from_golden, make_cfg, params_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)
OUTPUTS = ("count", "nearest", "d2_nearest", "lists", "n_total")
SENTINEL = -77


def _engine(arrs, cfg, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    return eng


def _dp(a):
    return a.ctypes.data_as(_D) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(_I64P) if a is not None else None


def find(eng, px, py, r, want=OUTPUTS, cap=None):
    """(rc, outputs) of one raw bh_find_neighbors call.  r: a scalar (pr = NULL) or an array.
    Outputs not in `want` are passed as NULL; the given ones start filled with a sentinel, the
    list with `cap` entries (default: room for every pair)."""
    px = np.ascontiguousarray(px, dtype=np.float64)
    py = np.ascontiguousarray(py, dtype=np.float64)
    n = len(px)
    pr = None if np.ndim(r) == 0 else np.ascontiguousarray(r, dtype=np.float64)
    if cap is None:
        cap = n * max(eng.num_bodies(), 1)
    out = dict(count=np.full(n, SENTINEL, dtype=np.int64) if "count" in want else None,
               nearest=np.full(n, SENTINEL, dtype=np.int64) if "nearest" in want else None,
               d2_nearest=np.full(n, -7.0) if "d2_nearest" in want else None,
               offsets=np.full(n + 1, SENTINEL, dtype=np.int64) if "lists" in want else None,
               indices=np.full(max(cap, 1), SENTINEL, dtype=np.int64) if "lists" in want else None)
    total = ctypes.c_int64(SENTINEL)
    rc = eng._lib.bh_find_neighbors(
        eng._h, n, _dp(px), _dp(py), 0.0 if pr is not None else float(r), _dp(pr),
        _ip(out["count"]), _ip(out["nearest"]), _dp(out["d2_nearest"]), _ip(out["offsets"]),
        _ip(out["indices"]), cap, ctypes.byref(total) if "n_total" in want else None)
    out["n_total"] = total.value if "n_total" in want else None
    return rc, out


def assert_same(got, want, what="", lists=True):
    """Every output that `got` holds equals `want`'s (the checker's dict, or another call's)."""
    for k in ("count", "nearest", "offsets"):
        if got.get(k) is not None:
            assert np.array_equal(got[k], want[k]), f"{what}{k}"
    if got.get("d2_nearest") is not None:
        assert np.array_equal(got["d2_nearest"].view(np.int64),
                              np.asarray(want["d2_nearest"]).view(np.int64)), f"{what}d2_nearest"
    total = int(want["offsets"][-1])
    if got.get("n_total") is not None:
        assert got["n_total"] == total, f"{what}n_total"
    if lists and got.get("indices") is not None:
        assert np.array_equal(got["indices"][:total], want["indices"][:total]), f"{what}indices"
        assert np.all(got["indices"][total:] == SENTINEL), f"{what}indices past the total"


def assert_state(eng, st, what=""):
    for name, a, b in zip(FIELDS, eng.get_bodies(), st):
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"{what}{name}"


def check(arrs, cfg, px, py, r, eng=None):
    """One full call on a fresh engine (or `eng`) against the checker; returns the outputs."""
    own = eng is None
    eng = eng or _engine(arrs, cfg)
    idx, x, y, st, _ = candidates(arrs, cfg)
    rc, got = find(eng, px, py, r)
    assert rc == bh_amd.BH_OK, eng._lib.bh_last_error(eng._h)
    assert_same(got, brute(idx, x, y, px, py, r))
    assert_state(eng, st)
    if own:
        eng.close()
    return got


# ---- the default tree: two_disks(600, 200), its candidates and probes, made once ------------

CFG = make_cfg(theta=0.5)


@functools.lru_cache(maxsize=None)
def _tree():
    return scenes.two_disks(600, 200)


@functools.lru_cache(maxsize=None)
def _cand():
    return candidates(_tree(), CFG)


@functools.lru_cache(maxsize=None)
def _probes320():
    """make_probes' 300 plus 20 probes placed on bodies (positions after the build)."""
    px, py = make_probes(_tree(), CFG, 300, 23)
    st = _cand()[3]
    on = np.random.default_rng(29).choice(len(st[0]), 20, replace=False)
    return np.concatenate([px, st[0][on]]), np.concatenate([py, st[1][on]])


@functools.lru_cache(maxsize=None)
def _probes_many():
    """Probes for the largest count, in make_probes' mix (lists of 8192, one seed each: the mix
    draws its on-body probes without replacement)."""
    parts = [make_probes(_tree(), CFG, 8192, 31 + k) for k in range(-(-SHAPE_COUNTS[-1] // 8192))]
    return tuple(np.concatenate(p)[:SHAPE_COUNTS[-1]] for p in zip(*parts))


@functools.lru_cache(maxsize=None)
def _want_many():
    idx, x, y, _, _ = _cand()
    px, py = _probes_many()
    return brute(idx, x, y, px, py, 8.0)


def _prefix(want, n):
    """The checker's answer for the first n probes of a longer list."""
    total = int(want["offsets"][n])
    return dict(count=want["count"][:n], nearest=want["nearest"][:n],
                d2_nearest=want["d2_nearest"][:n], offsets=want["offsets"][:n + 1],
                indices=want["indices"][:total])


@pytest.mark.parametrize("r", [0.0, 0.5, 8.0, 50.0, math.inf])
def test_two_disks_radii_and_null_outputs(r):
    px, py = _probes320()
    idx, x, y, st, _ = _cand()
    want = brute(idx, x, y, px, py, r)
    eng = _engine(_tree(), CFG)
    rc, full = find(eng, px, py, r)
    assert rc == bh_amd.BH_OK
    assert_same(full, want)
    assert_state(eng, st)
    if r == 0.0:
        assert np.all(full["count"][300:] >= 1) and np.all(full["d2_nearest"][300:] == 0.0)
    if r == math.inf:
        assert np.all(full["count"] == len(idx))
    # every combination of NULL outputs agrees with the full call
    for k in range(len(OUTPUTS) + 1):
        for want_set in itertools.combinations(OUTPUTS, k):
            rc, part = find(eng, px, py, r, want=want_set)
            assert rc == bh_amd.BH_OK, want_set
            assert_same(part, full, f"{want_set}: ")
    eng.close()


def _jitter_scene(name):
    if name == "pair":  # two jittered bodies that stay in the tree (test_neighbors_ref)
        return jitter_pair(CFG), CFG
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    return tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z)


@pytest.mark.parametrize("name", ["jitter_306", "pair"])
def test_jitter_cluster(name):
    """Probes on and beside the bodies the build jitters -- where they were and where it left
    them: this is where a too-small reach loses a body."""
    arrs, cfg = _jitter_scene(name)
    idx, x, y, st, _ = candidates(arrs, cfg)
    moved = np.flatnonzero((st[0].view(np.int64) != arrs[0].view(np.int64)) |
                           (st[1].view(np.int64) != arrs[1].view(np.int64)))
    assert moved.size >= 2  # the scene does jitter
    cx, cy = st[0][moved], st[1][moved]
    rng = np.random.default_rng(37)
    ox, oy = rng.uniform(-5e-3, 5e-3, (2, 8, moved.size))
    px = np.concatenate([cx, cx + 1e-3, cx - 7e-4, arrs[0][moved], (cx + ox).ravel(), x[:8]])
    py = np.concatenate([cy, cy - 1e-3, cy + 7e-4, arrs[1][moved], (cy + oy).ravel(), y[:8]])
    found = 0
    for r in (5e-4, 1e-3, 2e-3, 1e-2):  # (a fresh engine each: every call builds, and jitters)
        found += int(check(arrs, cfg, px, py, r)["n_total"])
    assert found >= 4 * min(8, len(idx))
    if name == "pair":
        assert np.isin(moved, idx).all()


def test_outside_root_and_odd_probes():
    z = np.load(os.path.join(GOLDEN, "outside_153.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    cx, cy, h = root_cell(cfg)
    outside = np.flatnonzero((np.abs(arrs[0] - cx) >= h) | (np.abs(arrs[1] - cy) >= h))
    assert outside.size > 0
    px, py = make_probes(arrs, cfg, 120, 41)
    odd_x = [cx + 3 * h, cx - 2 * h, 2.0 ** 40, 1e300, -1e300, math.nan, cx, math.nan, cx, cx]
    odd_y = [cy, cy + 5 * h, 2.0 ** 40, 1e300, cy, cy, math.nan, math.nan, cy, cy]
    px = np.concatenate([px, arrs[0][outside], odd_x])  # probes on the out-of-root bodies too
    py = np.concatenate([py, arrs[1][outside], odd_y])
    n = len(px)
    got = check(arrs, cfg, px, py, 30.0)
    on_out = slice(120, 120 + outside.size)
    for j in range(120, 120 + outside.size):  # an out-of-root body is never found, not by r = 0
        assert not np.isin(outside, got["indices"][got["offsets"][j]:got["offsets"][j + 1]]).any()
    assert np.all(check(arrs, cfg, px, py, 0.0)["count"][on_out] == 0)
    radii = np.resize(np.array([math.nan, -1.0, 0.0, math.inf, 25.0, 1e300, -0.0, 3 * h]), n)
    got = check(arrs, cfg, px, py, radii)
    assert np.all(got["count"][np.isnan(radii) | (radii < 0)] == 0)
    assert np.all(got["count"][np.isnan(px) | np.isnan(py)] == 0)
    check(arrs, cfg, px, py, np.roll(radii, 3))


def _dozen():
    """Twelve bodies: the six of the checker's own case; 6 and 7, both of negative mass, alone in
    a cell of their own, so the internal node above them has mass 0 and hides them; 8 of negative
    mass beside 9 of positive mass (found); 10 of mass 0 beside 11."""
    x, y, vx, vy, m = six_bodies()
    x = np.concatenate([x, [2000.0, 2000.5, 1800.0, 1800.5, 400.0, 400.5]])
    y = np.concatenate([y, [700.0, 700.5, 100.0, 100.5, 100.0, 100.5]])
    m = np.concatenate([m, [-1.0, -2.0, -4.0, 5.0, 0.0, 6.0]])
    return x, y, np.zeros(12), np.zeros(12), m


def test_zero_and_negative_masses():
    arrs = _dozen()
    idx, x, y, st, _ = candidates(arrs, CFG)
    assert idx.tolist() == [0, 1, 2, 5, 8, 9, 11]  # 6 and 7 lie under a mass-0 internal node
    px = np.concatenate([arrs[0], arrs[0] + 0.25, [1200.0]])
    py = np.concatenate([arrs[1], arrs[1] + 0.25, [400.0]])
    for r in (0.0, 1.0, 400.0, math.inf):
        check(arrs, CFG, px, py, r)


def _shape_counts():
    """Probe counts 1, 63, 64, 65, the counts just below and at every change of the launch's
    lanes per wave up to 8192, and one count whose last workgroup is partial."""
    shape = [bh_amd.tracer_launch_shape(n) for n in range(1, 8193)]  # shape[n - 1]
    counts = {1, 63, 64, 65}
    for n in range(2, 8193):
        if shape[n - 1][0] != shape[n - 2][0]:
            counts |= {n - 1, n}
    # workgroups of several waves come with larger launches only: the first such count (by
    # bisection: one wave per workgroup below it), then the next whose last workgroup is partial
    lo, hi = 8192, 1 << 20
    assert bh_amd.tracer_launch_shape(lo)[1] == 1 < bh_amd.tracer_launch_shape(hi)[1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if bh_amd.tracer_launch_shape(mid)[1] == 1 else (lo, mid)
    n = hi
    while _last_group_waves(n) in (0, 1):
        n += 1
    return sorted(counts | {n})


def _last_group_waves(n):
    """Waves in the launch's last workgroup for n probes; 0: it is full."""
    bpw, wpb, _ = bh_amd.tracer_launch_shape(n)
    return (-(-n // bpw)) % wpb


SHAPE_COUNTS = _shape_counts()


def test_shape_counts_cover_a_partial_workgroup():
    assert {1, 63, 64, 65} <= set(SHAPE_COUNTS) and len(SHAPE_COUNTS) >= 8
    n = SHAPE_COUNTS[-1]
    assert bh_amd.tracer_launch_shape(n)[1] > 1 and _last_group_waves(n) > 1


@pytest.mark.parametrize("n", SHAPE_COUNTS)
def test_probe_counts(n):
    px, py = _probes_many()
    eng = _engine(_tree(), CFG)
    rc, got = find(eng, px[:n], py[:n], 8.0, cap=int(_want_many()["offsets"][n]))
    assert rc == bh_amd.BH_OK
    assert_same(got, _prefix(_want_many(), n))
    eng.close()


def test_capacity():
    px, py = _probes320()
    idx, x, y, st, _ = _cand()
    want = brute(idx, x, y, px, py, 8.0)
    total = int(want["offsets"][-1])
    assert total > 1
    eng = _engine(_tree(), CFG)
    rc, got = find(eng, px, py, 8.0, cap=total - 1)
    assert rc == bh_amd.BH_E_CAPACITY
    assert b"bh_find_neighbors" in eng._lib.bh_last_error(eng._h)
    assert_same(got, want, "too small: ", lists=False)
    assert np.all(got["indices"] == SENTINEL)  # untouched
    assert_state(eng, st)
    rc, got = find(eng, px, py, 8.0, cap=got["n_total"])
    assert rc == bh_amd.BH_OK
    assert_same(got, want, "re-call: ")
    rc, got = find(eng, px, py, 8.0, cap=0)
    assert rc == bh_amd.BH_E_CAPACITY and got["n_total"] == total
    # the Python mirror re-calls by itself
    res = eng.find_neighbors(px, py, 50.0, lists=True)
    big = brute(idx, x, y, px, py, 50.0)
    assert len(res[4]) == int(big["offsets"][-1]) > 8 * len(px)
    for g, k in zip(res, ("count", "nearest", "d2_nearest", "offsets", "indices")):
        assert np.array_equal(g, big[k]), k
    count, nearest, d2 = eng.find_neighbors(px, py, np.full(len(px), 8.0))
    assert np.array_equal(count, want["count"]) and np.array_equal(nearest, want["nearest"])
    none, nearest, d2 = eng.find_neighbors(px, py, 8.0, counts=False)
    assert none is None and np.array_equal(nearest, want["nearest"])
    assert np.array_equal(d2, want["d2_nearest"])
    eng.close()


def test_no_probes_and_no_bodies():
    eng = _engine(_tree(), CFG)
    rc, got = find(eng, np.zeros(0), np.zeros(0), 1.0)
    assert rc == bh_amd.BH_OK and got["n_total"] == 0 and got["offsets"].tolist() == [0]
    assert_state(eng, _cand()[3])  # the build still happened
    total = ctypes.c_int64(SENTINEL)
    assert eng._lib.bh_find_neighbors(eng._h, 0, None, None, 1.0, None, None, None, None, None,
                                      None, 0, ctypes.byref(total)) == bh_amd.BH_OK
    assert total.value == 0
    eng.close()
    empty = tuple(np.zeros(0) for _ in range(5))
    eng = _engine(empty, CFG)
    px, py = np.array([1200.0, 3.0, math.nan]), np.array([400.0, 4.0, 1.0])
    rc, got = find(eng, px, py, math.inf)
    assert rc == bh_amd.BH_OK and got["n_total"] == 0
    assert got["count"].tolist() == [0, 0, 0] and got["offsets"].tolist() == [0, 0, 0, 0]
    assert got["nearest"].tolist() == [-1, -1, -1] and np.all(got["d2_nearest"] == math.inf)
    assert np.all(got["indices"] == SENTINEL)
    eng.close()


def _refusals():
    one = np.array([1000.0])
    d = one.ctypes.data_as(_D)
    off, ind = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.int64)
    o, i = off.ctypes.data_as(_I64P), ind.ctypes.data_as(_I64P)

    def call(lib, h, n=1, px=d, py=d, r=1.0, pr=None, offsets=None, indices=None, cap=0):
        return lib.bh_find_neighbors(h, n, px, py, r, pr, None, None, None, offsets, indices, cap,
                                     None)
    count = "bh_find_neighbors: n_probe must be in [0, 2^28]"
    keep = (one, off, ind)
    return [("negative", lambda lib, h: call(lib, h, n=-1), count, keep),
            ("too-many", lambda lib, h: call(lib, h, n=(1 << 28) + 1, px=None, py=None), count,
             keep),
            ("px-null", lambda lib, h: call(lib, h, px=None), "bh_find_neighbors: px or py is NULL",
             keep),
            ("py-null", lambda lib, h: call(lib, h, py=None), "bh_find_neighbors: px or py is NULL",
             keep),
            ("r-nan", lambda lib, h: call(lib, h, r=math.nan), "bh_find_neighbors: r must be >= 0",
             keep),
            ("r-negative", lambda lib, h: call(lib, h, r=-1.0),
             "bh_find_neighbors: r must be >= 0", keep),
            ("r-negative-no-probes", lambda lib, h: call(lib, h, n=0, r=-1.0),
             "bh_find_neighbors: r must be >= 0", keep),
            ("offsets-alone", lambda lib, h: call(lib, h, offsets=o, cap=4),
             "bh_find_neighbors: offsets or indices is NULL", keep),
            ("indices-alone", lambda lib, h: call(lib, h, indices=i, cap=4),
             "bh_find_neighbors: offsets or indices is NULL", keep),
            ("cap-negative", lambda lib, h: call(lib, h, offsets=o, indices=i, cap=-1),
             "bh_find_neighbors: cap must be >= 0", keep)]


_REFUSALS = _refusals()


@pytest.mark.parametrize("call,text", [r[1:3] for r in _REFUSALS], ids=[r[0] for r in _REFUSALS])
def test_refusal(call, text):
    arrs = six_bodies()
    eng = _engine(arrs, CFG)
    assert call(eng._lib, eng._h) == bh_amd.BH_E_INVALID
    assert eng._lib.bh_last_error(eng._h).decode() == text
    assert_state(eng, arrs)  # refused before anything was built
    eng.close()


def test_null_handle_and_negative_radius_with_pr():
    lib = bh_amd.load_library()
    one = np.array([1000.0])
    d = one.ctypes.data_as(_D)
    assert lib.bh_find_neighbors(None, 1, d, d, 1.0, None, None, None, None, None, None, 0,
                                 None) == bh_amd.BH_E_INVALID
    # with pr given, r is not used: a negative r is no refusal
    eng = _engine(six_bodies(), CFG)
    assert lib.bh_find_neighbors(eng._h, 1, d, d, -1.0, d, None, None, None, None, None, 0,
                                 None) == bh_amd.BH_OK
    eng.close()


def test_async_guard():
    eng = _engine(scenes.two_disks(300, 100), CFG)
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        rc, _ = find(eng, [1.0], [2.0], 5.0)
        assert rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    rc, got = find(eng, [1.0], [2.0], 5.0)
    assert rc == bh_amd.BH_OK and got["count"].tolist() == [0]
    eng.close()


def test_state_semantics_of_compute_accelerations():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    px, py = make_probes(arrs, cfg, 100, 43)
    a, b = _engine(arrs, cfg), _engine(arrs, cfg)
    assert find(a, px, py, 8.0)[0] == bh_amd.BH_OK
    b.compute_accelerations()
    assert_state(a, b.get_bodies(), "after the call: ")
    a.step(2)
    b.step(2)
    assert_state(a, b.get_bodies(), "after step(2): ")
    a.close()
    b.close()


def test_deterministic_and_multi_handle(monkeypatch):
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    px, py = _probes320()
    one = _engine(_tree(), CFG)
    two = _engine(_tree(), CFG, devices=[0, 0])
    assert two.multi_world() == 2
    rc, first = find(one, px, py, 8.0)
    assert rc == bh_amd.BH_OK
    for eng, what in ((one, "second call: "), (two, "multi handle: "), (two, "its second: ")):
        rc, again = find(eng, px, py, 8.0)
        assert rc == bh_amd.BH_OK
        assert_same(again, first, what)
    assert_state(two, one.get_bodies())
    one.step(2)
    two.step(2)
    assert_state(two, one.get_bodies(), "after step(2): ")
    assert two.neighbors_kernel_ms() > 0.0
    two.close()
    one.close()


def _ms(eng):
    ms = ctypes.c_double(-7.0)
    return eng._lib.bh_neighbors_kernel_ms(eng._h, ctypes.byref(ms)), ms.value


def test_stopwatch():
    eng = _engine(six_bodies(), CFG)
    fn = eng._lib.bh_neighbors_kernel_ms
    assert fn(eng._h, None) == bh_amd.BH_E_INVALID
    assert fn(None, ctypes.byref(ctypes.c_double(0.0))) == bh_amd.BH_E_INVALID
    assert _ms(eng) == (bh_amd.BH_OK, 0.0)  # nothing launched yet: exactly 0.0
    assert find(eng, np.zeros(0), np.zeros(0), 1.0)[0] == bh_amd.BH_OK
    assert _ms(eng) == (bh_amd.BH_OK, 0.0), "a call without a launch started the watch"
    assert find(eng, [700.0], [300.0], 1.0)[0] == bh_amd.BH_OK
    rc, first = _ms(eng)
    assert rc == bh_amd.BH_OK and math.isfinite(first) and first >= 0.0, (rc, first)
    assert find(eng, np.zeros(0), np.zeros(0), 1.0)[0] == bh_amd.BH_OK
    assert _ms(eng) == (bh_amd.BH_OK, first), "a call without a launch moved the watch"
    assert eng.neighbors_kernel_ms() == first
    eng.close()


def test_pick_returns_the_callers_body():
    arrs = _dozen()
    bodies = [bh_amd.Body(*(float(a[i]) for a in arrs)) for i in range(12)]
    pe = bh_amd.PhysicsEngine(bodies)
    idx, x, y, _, _ = candidates(arrs, make_cfg())
    for qx, qy, r in ((1010.0, 300.0, 10.0), (1010.0, 300.0, 9.0), (2000.2, 700.2, 5.0),
                      (1800.2, 100.2, 5.0), (400.0, 100.0, 0.5), (400.0, 100.0, 1.0),
                      (5000.0, 300.0, 50.0), (699.0, 301.0, math.inf)):
        want = int(brute(idx, x, y, [qx], [qy], r)["nearest"][0])
        got = pe.pick(qx, qy, r)
        if want < 0:
            assert got is None, (qx, qy, r)
        else:
            assert got is bodies[want], (qx, qy, r)
    assert pe.pick(1010.0, 300.0, 10.0) is bodies[1]   # the tie goes to the lower index
    assert pe.pick(2000.2, 700.2, 5.0) is None          # hidden under a mass-0 node
    assert pe.get_bodies() is bodies and len(bodies) == 12
