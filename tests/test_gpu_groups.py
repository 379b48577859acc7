"""GPU: bh_find_groups / bh_groups_kernel_ms / PhysicsEngine.groups.

Every value is compared exactly with the checker of tests/test_groups_ref.py: the candidate set
and the state after the build from the oracle's tree of the same start state, the definition of
friends-of-friends groups applied to it with numpy -- integers by array_equal, the sums on their
int64 view.  The calls go through the raw ABI so that every output can be given or withheld.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from test_groups_ref import (KNOWN, LINKS, catalogue, chain, checker, fof_all_pairs, fof_binned,
                             labels_of, spiral)
from test_neighbors_ref import FIELDS, candidates, jitter_pair, six_bodies
from test_potential_ref import cfg_from_golden, make_cfg, params_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)
OUTPUTS = ("label", "members", "groups", "summary")
SENTINEL = -77
CFG = make_cfg(theta=0.5)


def _engine(arrs, cfg=CFG, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    return eng


def find(eng, link, min_members=1, want=OUTPUTS, caps=None):
    """(rc, outputs) of one raw bh_find_groups call.  Outputs not in `want` are passed as NULL;
    the given ones start filled with a sentinel.  caps: (label, members, groups) capacities,
    default the number of bodies each."""
    n = eng.num_bodies()
    caps = (n, n, n) if caps is None else caps
    out = dict(
        label=np.full(max(caps[0], 1), SENTINEL, dtype=np.int64) if "label" in want else None,
        members=np.full(max(caps[1], 1), SENTINEL, dtype=np.int64) if "members" in want else None,
        groups=np.full(max(caps[2], 1) * 8, SENTINEL, dtype=np.int64).view(bh_amd.GROUP_DTYPE)
        if "groups" in want else None)
    sm = bh_amd.BhGroupsSummary(*([SENTINEL] * 6))
    ip = lambda a: a.ctypes.data_as(_I64P) if a is not None else None  # noqa: E731
    gp = out["groups"].ctypes.data_as(ctypes.POINTER(bh_amd.BhGroup)) \
        if out["groups"] is not None else None
    rc = eng._lib.bh_find_groups(eng._h, float(link), int(min_members), ip(out["label"]), caps[0],
                                 ip(out["members"]), caps[1], gp, caps[2],
                                 ctypes.byref(sm) if "summary" in want else None)
    out["summary"] = tuple(getattr(sm, f[0]) for f in sm._fields_) if "summary" in want else None
    return rc, out


def _untouched(a):
    return np.all(a.view(np.int64) == SENTINEL)


def assert_same(got, want, what=""):
    """Every output that `got` holds equals `want`'s (the checker's catalogue, or another
    call's), bit for bit; what lies past the answer still holds the sentinel."""
    n_bodies, n_in, _, n_groups = want["summary"][:4]
    if got.get("summary") is not None:
        assert got["summary"] == tuple(want["summary"]), f"{what}summary"
    if got.get("label") is not None:
        n = len(want["label"])
        assert np.array_equal(got["label"][:n], want["label"][:n]), f"{what}label"
        assert _untouched(got["label"][n:]), f"{what}label past N"
    if got.get("members") is not None:
        assert np.array_equal(got["members"][:n_in], want["members"][:n_in]), f"{what}members"
        assert _untouched(got["members"][n_in:]), f"{what}members past n_in_tree"
    if got.get("groups") is not None:
        a, b = got["groups"][:n_groups], want["groups"][:n_groups]
        for f in bh_amd.GROUP_DTYPE.names:
            assert np.array_equal(a[f].view(np.int64), b[f].view(np.int64)), f"{what}groups.{f}"
        assert _untouched(got["groups"][n_groups:]), f"{what}groups past n_groups"


def assert_state(eng, st, what=""):
    for name, a, b in zip(FIELDS, eng.get_bodies(), st):
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), f"{what}{name}"


def check(arrs, cfg, link, min_members=1, fof=fof_all_pairs):
    """One full call on a fresh engine against the checker; returns the outputs."""
    eng = _engine(arrs, cfg)
    want, st = checker(arrs, cfg, link, min_members, fof)
    rc, got = find(eng, link, min_members)
    assert rc == bh_amd.BH_OK, eng._lib.bh_last_error(eng._h)
    assert_same(got, want)
    assert_state(eng, st)
    eng.close()
    return got


# ---- the default tree: two_disks(600, 200) ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tree():
    return scenes.two_disks(600, 200)


@functools.lru_cache(maxsize=None)
def _cand():
    return candidates(_tree(), CFG)


@functools.lru_cache(maxsize=None)
def _labels(link):
    idx, x, y, _, _ = _cand()
    return labels_of(len(_tree()[0]), idx, fof_all_pairs(idx, x, y, link))


@pytest.mark.parametrize("link", LINKS)
def test_two_disks_links_and_null_outputs(link):
    st = _cand()[3]
    eng = _engine(_tree())
    for min_members in (1, 2, 8):
        want = catalogue(_labels(link), st, min_members)
        rc, full = find(eng, link, min_members)
        assert rc == bh_amd.BH_OK
        assert_same(full, want, f"min_members {min_members}: ")
        if min_members == 1:
            assert (full["summary"][2], full["summary"][5]) == KNOWN[link]
        assert_state(eng, st)
        for without in OUTPUTS:  # each output withheld in turn
            rc, part = find(eng, link, min_members, want=[o for o in OUTPUTS if o != without])
            assert rc == bh_amd.BH_OK, without
            assert_same(part, want, f"without {without}: ")
    # an array that is NULL is not asked for, whatever its cap
    rc, part = find(eng, link, 1, want=("summary",), caps=(5, 5, 5))
    assert rc == bh_amd.BH_OK
    assert part["summary"] == tuple(catalogue(_labels(link), st, 1)["summary"])
    eng.close()


# ---- odd bodies ---------------------------------------------------------------------------------

def test_six_bodies():
    arrs = six_bodies()
    got = check(arrs, CFG, 20.0)
    assert got["label"][:6].tolist() == [0, 1, 1, -1, -1, 5]  # 1-2: exactly 20 apart, `<=`
    assert got["members"][:4].tolist() == [0, 1, 2, 5]  # not 3 (outside) nor 4 (mass 0)
    got = check(arrs, CFG, math.nextafter(20.0, 0.0))
    assert got["label"][:6].tolist() == [0, 1, 2, -1, -1, 5]
    for link in (0.0, 299.0, 301.0, 1e4, math.inf):
        for min_members in (1, 2, 5):
            check(arrs, CFG, link, min_members)


def test_jitter_pair_links_by_the_positions_after_the_build():
    arrs = jitter_pair(CFG)
    idx, x, y, st, _ = candidates(arrs, CFG)
    a, b = int(np.flatnonzero(idx == 6)[0]), int(np.flatnonzero(idx == 7)[0])
    dx, dy = x[a] - x[b], y[a] - y[b]
    d2 = dx * dx + dy * dy
    above = math.sqrt(d2)
    while above * above < d2:
        above = math.nextafter(above, math.inf)
    below = above
    while below * below >= d2:
        below = math.nextafter(below, 0.0)
    before = math.hypot(arrs[0][6] - arrs[0][7], arrs[1][6] - arrs[1][7])
    assert abs(before - above) > 1e-4  # the build did change their distance
    got = check(arrs, CFG, above)
    assert got["label"][6] == got["label"][7] == 6
    got = check(arrs, CFG, below)
    assert (got["label"][6], got["label"][7]) == (6, 7)


def test_jitter_306():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    n_in = set()
    for link in (0.0, 1e-3, 5.0, 40.0):  # (a fresh engine each: every call builds, and jitters)
        got = check(arrs, cfg, link, 2)
        n_in.add(got["summary"][1])
    assert len(n_in) == 1 and 0 < n_in.pop() < len(arrs[0])  # the jitter dropped bodies


# ---- a chain, the union-find's worst case --------------------------------------------------------

def test_chain():
    arrs = chain()
    got = check(arrs, CFG, 1.0, fof=fof_binned)
    assert got["summary"] == (1000, 1000, 1, 1, 0, 1000)
    assert np.all(got["label"][:1000] == 0) and arrs[0][0] != 600.0  # label 0 is not the first slot
    assert got["groups"]["count"][0] == 1000 and got["groups"]["mass"][0] == 1000.0
    got = check(arrs, CFG, math.nextafter(1.0, 0.0), fof=fof_binned)
    assert got["summary"] == (1000, 1000, 1000, 1000, 0, 1)
    assert np.array_equal(got["label"][:1000], np.arange(1000))
    check(arrs, CFG, 1.0, 2, fof=fof_binned)
    check(arrs, CFG, math.nextafter(1.0, 0.0), 2, fof=fof_binned)


def test_spiral():
    arrs = spiral()
    got = check(arrs, CFG, 1.0, 2, fof=fof_binned)
    assert got["summary"] == (4000, 4000, 1, 1, 0, 4000)
    got = check(arrs, CFG, math.nextafter(1.0, 0.0), fof=fof_binned)
    assert got["summary"][2:] == (4000, 4000, 0, 1)
    check(arrs, CFG, 2.0, fof=fof_binned)  # the arms join


# ---- launch shapes ----------------------------------------------------------------------------------

def _last_group_waves(n):
    """Waves in the launch's last workgroup for n lanes; 0: it is full."""
    bpw, wpb, _ = bh_amd.tracer_launch_shape(n)
    return (-(-n // bpw)) % wpb


def _shape_counts():
    """Body counts 1, 2, 63, 64, 65, the counts just below and at every change of the launch's
    (lanes per wave, waves per workgroup) up to 8193, the first count with more than one wave per
    workgroup and the next one whose last workgroup is partial."""
    shape = [bh_amd.tracer_launch_shape(n)[:2] for n in range(1, 8194)]  # shape[n - 1]
    counts = {1, 2, 63, 64, 65}
    for n in range(2, 8194):
        if shape[n - 1] != shape[n - 2]:
            counts |= {n - 1, n}
    lo, hi = 8193, 1 << 20
    assert bh_amd.tracer_launch_shape(lo)[1] == 1 < bh_amd.tracer_launch_shape(hi)[1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if bh_amd.tracer_launch_shape(mid)[1] == 1 else (lo, mid)
    n = hi + 1
    while _last_group_waves(n) in (0, 1):
        n += 1
    return sorted(counts | {hi, n})


SHAPE_COUNTS = _shape_counts()
N_UNIFORM = 70000


@functools.lru_cache(maxsize=None)
def _uniform():
    return scenes.uniform(N_UNIFORM, 0.5, seed=11)


def test_shape_counts_cover_a_partial_workgroup():
    assert {1, 2, 63, 64, 65} <= set(SHAPE_COUNTS) and len(SHAPE_COUNTS) >= 9
    n = SHAPE_COUNTS[-1]
    assert n <= N_UNIFORM
    assert bh_amd.tracer_launch_shape(n)[1] > 1 and _last_group_waves(n) > 1
    assert bh_amd.tracer_launch_shape(SHAPE_COUNTS[-2])[1] > 1


@pytest.mark.parametrize("n", SHAPE_COUNTS)
def test_body_counts(n):
    """The first n bodies of a uniform scene at a link length near the percolation threshold
    (about 4 friends each): groups of every size.  The scene's closest pair is far above the
    jitter cell, so S is every body and the build moves nothing -- asserted -- and the checker
    runs on the input itself."""
    arrs = tuple(a[:n] for a in _uniform())
    link = 6.0 * math.sqrt(N_UNIFORM / n)
    label = fof_binned(np.arange(n), arrs[0], arrs[1], link)
    want = catalogue(label, arrs, 2)
    assert want["summary"][1] == n
    if n >= 1024:
        assert want["summary"][2] > 30 and 100 < want["summary"][5] < n // 4
    eng = _engine(arrs)
    rc, got = find(eng, link, 2, caps=(n, n, want["summary"][3]))
    assert rc == bh_amd.BH_OK, eng._lib.bh_last_error(eng._h)
    assert_state(eng, arrs, "the build moved a body: ")
    assert_same(got, want)
    eng.close()


# ---- capacity, empty cases, refusals ----------------------------------------------------------------

def test_capacity():
    st = _cand()[3]
    want = catalogue(_labels(8.0), st, 2)
    exact = (800, want["summary"][1], want["summary"][3])
    assert all(c > 1 for c in exact)
    eng = _engine(_tree())
    for k in range(3):
        caps = tuple(c - 1 if i == k else c for i, c in enumerate(exact))
        rc, got = find(eng, 8.0, 2, caps=caps)
        assert rc == bh_amd.BH_E_CAPACITY, k
        assert b"bh_find_groups" in eng._lib.bh_last_error(eng._h)
        assert got["summary"] == tuple(want["summary"])
        for name in ("label", "members", "groups"):
            assert _untouched(got[name]), (k, name)
        assert_state(eng, st)
    rc, got = find(eng, 8.0, 2, caps=exact)
    assert rc == bh_amd.BH_OK
    assert_same(got, want, "re-call: ")
    # the Python mirror sizes the catalogue by itself
    summary, label, groups, members = eng.find_groups(8.0, 2, members=True)
    assert tuple(summary.__dict__.values()) == tuple(want["summary"])
    assert np.array_equal(label, want["label"]) and np.array_equal(members, want["members"])
    assert groups.tobytes() == want["groups"].tobytes()
    summary, label, groups = eng.find_groups(8.0, 8, labels=False)
    assert label is None and groups.tobytes() == catalogue(_labels(8.0), st, 8)["groups"].tobytes()
    eng.close()


def _ms(eng):
    ms = ctypes.c_double(-7.0)
    return eng._lib.bh_groups_kernel_ms(eng._h, ctypes.byref(ms)), ms.value


def test_empty_cases():
    empty = tuple(np.zeros(0) for _ in range(5))
    outside = (np.array([5000.0, -900.0, 6000.0]), np.array([300.0, 100.0, 9000.0]), np.zeros(3),
               np.zeros(3), np.ones(3))
    assert len(candidates(outside, CFG)[0]) == 0
    for arrs, n in ((empty, 0), (outside, 3)):
        eng = _engine(arrs)
        assert _ms(eng) == (bh_amd.BH_OK, 0.0)
        rc, got = find(eng, 10.0, 1)
        assert rc == bh_amd.BH_OK
        assert got["summary"] == (0, 0, 0, 0, -1, 0)
        assert got["label"][:n].tolist() == [-1] * n and _untouched(got["label"][n:])
        assert _untouched(got["members"]) and _untouched(got["groups"])
        assert _ms(eng) == (bh_amd.BH_OK, 0.0), "a call on an empty S started the watch"
        eng.close()
    # ... and after a call that did launch, an empty S leaves its reading
    eng = _engine(six_bodies())
    assert find(eng, 10.0)[0] == bh_amd.BH_OK
    rc, first = _ms(eng)
    assert rc == bh_amd.BH_OK and first > 0.0
    for arrs in (outside, empty):
        eng.reset_bodies(*arrs)
        rc, got = find(eng, 10.0)
        assert rc == bh_amd.BH_OK and got["summary"] == (0, 0, 0, 0, -1, 0)
        assert _ms(eng) == (bh_amd.BH_OK, first), "a call on an empty S moved the watch"
    eng.close()


_REFUSALS = [
    ("link-nan", dict(link=math.nan), "bh_find_groups: link must be >= 0"),
    ("link-negative", dict(link=-1.0), "bh_find_groups: link must be >= 0"),
    ("min-members-zero", dict(min_members=0), "bh_find_groups: min_members must be >= 1"),
    ("label-cap-negative", dict(caps=(-1, 6, 6)), "bh_find_groups: label_cap must be >= 0"),
    ("members-cap-negative", dict(caps=(6, -1, 6)), "bh_find_groups: members_cap must be >= 0"),
    ("groups-cap-negative", dict(caps=(6, 6, -1)), "bh_find_groups: groups_cap must be >= 0"),
]


@pytest.mark.parametrize("kw,text", [r[1:] for r in _REFUSALS], ids=[r[0] for r in _REFUSALS])
def test_refusal(kw, text):
    arrs = six_bodies()
    eng = _engine(arrs)
    args = dict(link=1.0, min_members=1, caps=(6, 6, 6))
    args.update(kw)
    rc, got = find(eng, args["link"], args["min_members"], caps=args["caps"])
    assert rc == bh_amd.BH_E_INVALID
    assert eng._lib.bh_last_error(eng._h).decode() == text
    assert got["summary"] == (SENTINEL,) * 6 and _untouched(got["label"])
    assert_state(eng, arrs)  # refused before anything was built
    # a negative cap is refused also where its array is NULL
    if "caps" in kw:
        rc, _ = find(eng, 1.0, 1, want=("summary",), caps=args["caps"])
        assert rc == bh_amd.BH_E_INVALID
    eng.close()


def test_async_guard():
    arrs = scenes.two_disks(300, 100)
    eng = _engine(arrs)
    eng.set_mirror(True, buffers=2)
    eng.step_begin(1)
    try:
        rc, _ = find(eng, 5.0)
        assert rc == bh_amd.BH_E_STATE
    finally:
        eng.step_end()
    rc, got = find(eng, 5.0)
    assert rc == bh_amd.BH_OK and got["summary"][0] == eng.num_bodies()
    eng.close()


# ---- state semantics, determinism, the multi-device handle -----------------------------------------

def test_state_semantics_of_compute_accelerations():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    a, b = _engine(arrs, cfg), _engine(arrs, cfg)
    assert find(a, 8.0)[0] == bh_amd.BH_OK
    b.compute_accelerations()
    assert_state(a, b.get_bodies(), "after the call: ")
    a.step(2)
    b.step(2)
    assert_state(a, b.get_bodies(), "after step(2): ")
    a.close()
    b.close()


def test_carried_tree_answers_for_the_state_it_shows():
    """After step(1) the engine may carry the next tree: the call answers for the bodies that
    get_bodies() shows after it, velocities included (the momentum sums)."""
    eng = _engine(_tree())
    eng.step(1)
    rc, got = find(eng, 8.0, 2)
    assert rc == bh_amd.BH_OK
    st = eng.get_bodies()
    n = len(st[0])
    in_tree = np.flatnonzero(got["label"][:n] >= 0)
    assert len(in_tree) == got["summary"][1] > 700
    label = labels_of(n, in_tree, fof_binned(in_tree, st[0][in_tree], st[1][in_tree], 8.0))
    assert_same(got, catalogue(label, st, 2))
    assert np.any(got["groups"]["px"][:got["summary"][3]] != 0.0)
    eng.close()


def test_deterministic_and_multi_handle(monkeypatch):
    monkeypatch.setenv("BH_MULTI_MIN_BODIES", "0")  # (small lists would step on one engine)
    one = _engine(_tree())
    other = _engine(_tree())
    two = _engine(_tree(), devices=[0, 0])
    assert two.multi_world() == 2
    rc, first = find(one, 8.0, 2)
    assert rc == bh_amd.BH_OK
    assert_same(first, catalogue(_labels(8.0), _cand()[3], 2))
    for eng, what in ((one, "second call: "), (other, "second engine: "), (two, "multi handle: "),
                      (two, "its second: ")):
        rc, again = find(eng, 8.0, 2)
        assert rc == bh_amd.BH_OK
        for name in ("label", "members", "groups"):
            assert again[name].tobytes() == first[name].tobytes(), what + name
        assert again["summary"] == first["summary"], what
    assert_state(two, one.get_bodies())
    one.step(2)
    two.step(2)
    assert_state(two, one.get_bodies(), "after step(2): ")
    assert two.groups_kernel_ms() > 0.0
    for eng in (two, other, one):
        eng.close()


def test_relabelling_under_a_permuted_caller_order():
    arrs = _tree()
    n = len(arrs[0])
    perm = np.random.default_rng(13).permutation(n)  # body perm[k] of the list becomes body k
    eng = _engine(tuple(a[perm] for a in arrs))
    rc, got = find(eng, 8.0)
    assert rc == bh_amd.BH_OK
    eng.close()
    base = _labels(8.0)
    # the same partition: body perm[k]'s group is the image of body k's new group
    pos = np.empty(n, dtype=np.int64)
    pos[perm] = np.arange(n)  # old index -> new index
    want = np.full(n, -1, dtype=np.int64)
    for lab in np.unique(base[base >= 0]):
        olds = np.flatnonzero(base == lab)
        want[pos[olds]] = pos[olds].min()
    assert np.array_equal(got["label"][:n], want)
    assert got["summary"][2] == len(np.unique(base[base >= 0]))


# ---- the stopwatch and the drop-in --------------------------------------------------------------------

def test_stopwatch():
    eng = _engine(six_bodies())
    fn = eng._lib.bh_groups_kernel_ms
    assert fn(eng._h, None) == bh_amd.BH_E_INVALID
    assert _ms(eng) == (bh_amd.BH_OK, 0.0)  # nothing launched yet: exactly 0.0
    assert find(eng, 20.0)[0] == bh_amd.BH_OK
    rc, first = _ms(eng)
    assert rc == bh_amd.BH_OK and math.isfinite(first) and first > 0.0, (rc, first)
    one = np.array([700.0])
    d = one.ctypes.data_as(_D)
    cnt = np.zeros(1, dtype=np.int64)
    assert eng._lib.bh_find_neighbors(eng._h, 1, d, d, 5.0, None, cnt.ctypes.data_as(_I64P), None,
                                      None, None, None, 0, None) == bh_amd.BH_OK
    assert _ms(eng) == (bh_amd.BH_OK, first), "bh_find_neighbors moved the groups' watch"
    assert eng.groups_kernel_ms() == first
    eng.close()


def test_physics_engine_groups_returns_the_callers_bodies():
    arrs = tuple(a.copy() for a in six_bodies())
    bodies = [bh_amd.Body(*(float(a[i]) for a in arrs)) for i in range(6)]
    pe = bh_amd.PhysicsEngine(bodies)
    for link, min_members in ((20.0, 2), (20.0, 1), (19.0, 2), (1e4, 2)):
        want, _ = checker(arrs, make_cfg(), link, min_members)
        got = pe.groups(link, min_members)
        assert len(got) == len(want["groups"])
        for grp, rec in zip(got, want["groups"]):
            ids = want["members"][rec["first"]:rec["first"] + rec["count"]]
            assert len(grp) == len(ids)
            assert all(b is bodies[int(c)] for b, c in zip(grp, ids))
    assert [len(g) for g in pe.groups(20.0)] == [2] and pe.groups(20.0)[0][0] is bodies[1]
    assert pe.get_bodies() is bodies and len(bodies) == 6
