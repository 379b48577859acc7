"""GPU: tracers (bh_set_tracers and the calls around it) stepped inside bh_step.

Every value check is bit-exact: the tracers against the checkers of tests/test_tracers_ref.py
(the oracle's own step() with a fresh body per tracer), the bodies against oracle.Oracle run on
the bodies alone.  The reference of the default scene is computed once and shared; a tracer's
result depends neither on the number of tracers nor on its place in the list, so a test with
fewer tracers compares against a prefix of it.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import bh_amd
import oracle
from bh_amd import scenes
from test_field_ref import FIELDS, make_probes, root_cell
from test_potential_ref import cfg_from_golden, make_cfg, params_of
from test_tracers_ref import (oracle_with_appended, outside_tracers, tracer_steps,
                              tracer_steps_vec)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_D = ctypes.POINTER(ctypes.c_double)
_U32 = ctypes.POINTER(ctypes.c_uint32)
TNAMES = ("tx", "ty", "tvx", "tvy")


def _engine(arrs, cfg, tr=None):
    eng = bh_amd.Engine(params_of(cfg), device=0)
    eng.reset_bodies(*arrs)
    if tr is not None:
        eng.set_tracers(*tr)
    return eng


def _assert_bits(got, want, what, nan_equal=False):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    diff = got.view(np.int64) != want.view(np.int64)
    if nan_equal:
        diff &= ~(np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(diff)
    assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {bad[:5]}: "
                           f"{got[bad[:3]]} vs {want[bad[:3]]}")


def _assert_tracers(eng, want, what="", n=None, nan_equal=False):
    got = eng.get_tracers()
    for name, g, w in zip(TNAMES, got, want):
        _assert_bits(g, w if n is None else w[:n], what + name, nan_equal)


def _assert_bodies(eng, want, what=""):
    got = eng.get_bodies()
    for name, g, w in zip(FIELDS, got, want):
        _assert_bits(g, w, what + name)


def _oracle_bodies(arrs, cfg, k):
    ref = oracle.Oracle(*arrs, p=oracle.params(**cfg))
    ref.step(k)
    out = ref.get_bodies()
    ref.close()
    return out


def _with_velocities(tx, ty, seed, speed=30.0):
    rng = np.random.default_rng(seed)
    return tx, ty, rng.uniform(-speed, speed, len(tx)), rng.uniform(-speed, speed, len(tx))


@functools.lru_cache(maxsize=None)
def _scene():
    return scenes.two_disks(600, 200)


@functools.lru_cache(maxsize=None)
def _tracers():
    """600 tracers of the probe mix: inside the root cell, clumped at a disk centre, outside the
    root cell and on bodies, with velocities."""
    return _with_velocities(*make_probes(_scene(), make_cfg(theta=0.5), 600, 7), 8)


@functools.lru_cache(maxsize=None)
def _reference(theta, n, k):
    """Checker 1 for the first n default tracers on the default scene, and the C oracle's bodies
    of the scene alone, after k steps."""
    cfg = make_cfg(theta=theta)
    tr = tuple(a[:n] for a in _tracers())
    want_t, want_b = tracer_steps(_scene(), cfg, *tr, k)
    alone = _oracle_bodies(_scene(), cfg, k)
    for name, a, b in zip(FIELDS, want_b, alone):  # (the checker's bodies are the oracle's)
        _assert_bits(a, b, "checker " + name)
    return want_t, alone


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 600])
def test_tracer_counts(n):
    """Wave boundaries of the launch, two steps in one call; the bodies are what they are
    without tracers."""
    cfg = make_cfg(theta=0.5)
    eng = _engine(_scene(), cfg, tuple(a[:n] for a in _tracers()))
    assert eng.num_tracers() == n
    eng.step(2)
    want_t, want_b = _reference(0.5, 600, 2)
    _assert_tracers(eng, want_t, n=n)
    _assert_bodies(eng, want_b)
    assert eng.num_tracers() == n
    eng.close()


def _first_n(pred, lo, hi):
    """The smallest n in (lo, hi] with pred(n), pred monotone."""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


@functools.lru_cache(maxsize=None)
def _full_wave_sizes():
    """From the launch's own shape function: the smallest n with 64 tracers per wave, that n + 64,
    and the smallest n above it at which the waves per workgroup change again."""
    shape = bh_amd.tracer_launch_shape
    assert shape(1)[0] < 64 and shape(1 << 24)[0] == 64
    n64 = _first_n(lambda n: shape(n)[0] == 64, 1, 1 << 24)
    w0 = shape(n64 + 64)[1]
    assert shape(1 << 24)[1] != w0
    nw = _first_n(lambda n: shape(n)[1] != w0, n64 + 64, 1 << 24)
    return n64, n64 + 64, nw


@functools.lru_cache(maxsize=None)
def _small_tree():
    arrs = scenes.two_disks(75, 25)
    assert len(arrs[0]) == 100
    return arrs


@functools.lru_cache(maxsize=None)
def _full_wave_reference():
    """Checker 2 for the largest of the full-wave sizes on the 100-body tree, one step; the
    smaller sizes are prefixes of it."""
    cfg = make_cfg(theta=0.5)
    n = max(_full_wave_sizes())
    rng = np.random.default_rng(21)
    cx, cy, h = root_cell(cfg)
    tx = rng.uniform(cx - 1.2 * h, cx + 1.2 * h, n)  # (~30 % outside the root cell)
    ty = rng.uniform(cy - 1.2 * h, cy + 1.2 * h, n)
    on = rng.choice(n, 2000, replace=False)
    tx[on] = _small_tree()[0][on % 100]
    ty[on] = _small_tree()[1][on % 100]
    tr = _with_velocities(tx, ty, 22)
    want_t, want_b = tracer_steps_vec(_small_tree(), cfg, *tr, 1)
    return tr, want_t, want_b


@pytest.mark.parametrize("which", [0, 1, 2])
def test_full_wave_shapes(which):
    n = _full_wave_sizes()[which]
    bpw, wpb, _ = bh_amd.tracer_launch_shape(n)
    assert bpw == 64
    if which == 2:
        assert wpb != bh_amd.tracer_launch_shape(n - 1)[1]
    tr, want_t, want_b = _full_wave_reference()
    eng = _engine(_small_tree(), make_cfg(theta=0.5), tuple(a[:n] for a in tr))
    eng.step(1)
    _assert_tracers(eng, want_t, n=n)
    _assert_bodies(eng, want_b)
    eng.close()


@pytest.mark.parametrize("theta", [0.0, 0.2, 1.0, 1.6])
def test_theta_sweep(theta):
    """theta = 0 is the non-pipelined step: the bodies by the all-pairs kernel, the tracers by
    the same walk, which opens every node."""
    cfg = make_cfg(theta=theta)
    n = 130
    eng = _engine(_scene(), cfg, tuple(a[:n] for a in _tracers()))
    eng.step(2)
    want_t, want_b = _reference(theta, n, 2)
    _assert_tracers(eng, want_t)
    _assert_bodies(eng, want_b)
    eng.close()


def test_call_grouping():
    """k steps in one call = k one-step calls, with or without field and acceleration queries
    between them (their builds are the ones the next step would make)."""
    cfg = make_cfg(theta=0.5)
    tr = tuple(a[:130] for a in _tracers())
    want_t, want_b = _reference(0.5, 130, 3)
    one = _engine(_scene(), cfg, tr)
    one.step(3)
    _assert_tracers(one, want_t, "step(3) ")
    _assert_bodies(one, want_b, "step(3) ")
    one.close()
    single = _engine(_scene(), cfg, tr)
    for _ in range(3):
        single.step(1)
    _assert_tracers(single, want_t, "3 x step(1) ")
    _assert_bodies(single, want_b, "3 x step(1) ")
    single.close()
    mixed = _engine(_scene(), cfg, tr)
    px, py = make_probes(_scene(), cfg, 50, 9)
    mixed.compute_field(px, py)
    mixed.step(1)
    mixed.compute_field(px, py)
    mixed.step(1)
    mixed.compute_accelerations()
    mixed.step(1)
    mixed.compute_accelerations()
    _assert_tracers(mixed, want_t, "mixed ")
    mixed.close()


def test_reorder_interval_and_list_order():
    """2R + 1 steps cross two re-orderings of the lane map; the same tracers in a permuted list
    give the same results, permuted."""
    R = bh_amd.tracer_launch_shape(200)[2]
    arrs = scenes.two_disks(225, 75)
    assert len(arrs[0]) == 300
    cfg = make_cfg(theta=0.5)
    tr = _with_velocities(*make_probes(arrs, cfg, 200, 13), 14)
    perm = np.random.default_rng(15).permutation(200)
    k = 2 * R + 1
    a = _engine(arrs, cfg, tr)
    a.step(k)
    b = _engine(arrs, cfg, tuple(np.ascontiguousarray(v[perm]) for v in tr))
    for _ in range(k):  # (and one call per step: the map's age is carried across calls)
        b.step(1)
    got_a, got_b = a.get_tracers(), b.get_tracers()
    for name, u, v in zip(TNAMES, got_a, got_b):
        _assert_bits(v, u[perm], "permuted " + name)
    _assert_bodies(a, _oracle_bodies(arrs, cfg, k))
    _assert_bodies(b, a.get_bodies())
    # the first steps against the checker (its cost grows with every step)
    want_t, _ = tracer_steps(arrs, cfg, *tr, 2)
    c = _engine(arrs, cfg, tr)
    c.step(2)
    _assert_tracers(c, want_t)
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("case", ["no_bodies", "all_outside", "one_body"])
def test_empty_trees(case):
    cfg = make_cfg(theta=0.5)
    cx, cy, h = root_cell(cfg)
    if case == "no_bodies":
        arrs = tuple(np.zeros(0) for _ in range(5))
    elif case == "all_outside":
        arrs = (np.array([cx + h + 5.0, cx - h - 7.0, cx]), np.array([cy, cy + 3.0, cy + h + 9.0]),
                np.array([1.0, -2.0, 0.5]), np.array([0.5, 0.25, -1.0]), np.array([3.0, 5.0, 7.0]))
    else:
        arrs = (np.array([700.0]), np.array([300.0]), np.array([1.0]), np.array([-2.0]),
                np.array([900.0]))
    tr = (np.array([10.0, 700.0, cx + h + 5.0, 650.0]), np.array([20.0, 300.0, cy, 310.0]),
          np.array([-0.0, 2.0, -0.0, 0.0]), np.array([1.0, -0.0, -0.0, -3.0]))
    eng = _engine(arrs, cfg, tr)
    eng.step(2)
    want_t, want_b = tracer_steps(arrs, cfg, *tr, 2)
    _assert_tracers(eng, want_t, case + " ")
    _assert_bodies(eng, want_b, case + " ")
    if case != "one_body":  # nothing in any tree: -0.0 + 0.0 = +0.0, straight lines
        got = eng.get_tracers()
        for v in got[2:]:  # no -0.0 is left
            assert not (np.signbit(v) & (v == 0.0)).any()
        _assert_bits(got[0], tr[0] + (tr[2] + 0.0) * cfg["dt"] + (tr[2] + 0.0) * cfg["dt"], "x")
    eng.close()


def test_ieee_path():
    """soft2 = 0 and tracers at 2^40, 1e300 and NaN leave the fast path; no tracer coincides
    with a body or a centre of mass, so every other value is finite."""
    arrs = _scene()
    cfg = make_cfg(theta=0.5, soft2=0.0)
    tx, ty = make_probes(arrs, cfg, 200, 11, on_bodies=False)
    tx[-3], ty[-3] = 2.0 ** 40, -(2.0 ** 40)
    tx[-2], ty[-2] = 1e300, 1e300
    tx[-1], ty[-1] = np.nan, 400.0
    tr = _with_velocities(tx, ty, 12)
    want_t, want_b = tracer_steps_vec(arrs, cfg, *tr, 2)
    assert all(np.all(np.isfinite(w[:-1])) for w in want_t) and np.isnan(want_t[0][-1])
    eng = _engine(arrs, cfg, tr)
    eng.step(2)
    _assert_tracers(eng, want_t, nan_equal=True)
    _assert_bodies(eng, want_b)
    eng.close()


def test_jitter_scene():
    z = np.load(os.path.join(GOLDEN, "jitter_306.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    tr = _with_velocities(*make_probes(arrs, cfg, 130, 17), 18)
    want_t, want_b = tracer_steps(arrs, cfg, *tr, 2)
    eng = _engine(arrs, cfg, tr)
    eng.step(2)
    _assert_tracers(eng, want_t)
    _assert_bodies(eng, want_b)
    _assert_bodies(eng, _oracle_bodies(arrs, cfg, 2), "oracle ")
    eng.close()


def test_merging_leaves_the_tracers_alone():
    """Tracers within mergeMinDist of a heavy body while the merge rule removes bodies: never
    victims, not counted in N."""
    arrs = scenes.config_scene("c1_baseline")
    cfg = make_cfg(theta=0.5)
    heavy = int(np.argmax(arrs[4]))
    assert arrs[4][heavy] > cfg["merge_max_mass"]
    rng = np.random.default_rng(19)
    r, phi = rng.uniform(0.5, 7.5, 100), rng.uniform(0.0, 2.0 * np.pi, 100)
    tr = _with_velocities(arrs[0][heavy] + r * np.cos(phi), arrs[1][heavy] + r * np.sin(phi), 20)
    want_b = _oracle_bodies(arrs, cfg, 3)
    assert len(want_b[0]) < len(arrs[0])  # the scene merges within three steps
    want_t, chk_b = tracer_steps(arrs, cfg, *tr, 3)
    eng = _engine(arrs, cfg, tr)
    eng.step(3)
    assert eng.num_bodies() == len(want_b[0]) and eng.num_tracers() == 100
    _assert_tracers(eng, want_t)
    _assert_bodies(eng, want_b)
    _assert_bodies(eng, chk_b, "checker ")
    eng.close()


def _crowd():
    """The 520-heavy crowd of test_gpu_parity.test_merge_rule_more_pairs_than_the_mailbox."""
    rng = np.random.default_rng(77)
    nh = 520
    hx = 1000.0 + 20.0 * rng.random(nh)
    hy = 400.0 + 20.0 * rng.random(nh)
    hm = rng.uniform(4001.0, 6000.0, nh)
    field = scenes.uniform(3000, 0.5, seed=17)
    x = np.concatenate([hx, field[0]])
    y = np.concatenate([hy, field[1]])
    m = np.concatenate([hm, field[4]])
    perm = rng.permutation(len(x))
    arrs = tuple(a[perm] for a in (x, y, np.zeros(len(x)), np.zeros(len(x)), m))
    d2 = (hx[:, None] - x[None, :]) ** 2 + (hy[:, None] - y[None, :]) ** 2
    assert (d2 < 64.0).sum() - nh > max(65_536, 2 * len(x))  # the first step overflows
    return arrs


def test_replayed_call_steps_the_tracers_once():
    """The first step's candidate pairs overflow the merge mailbox: the call is replayed from
    its snapshot, tracers included.  Outside the root cell the tracers are what the C oracle
    makes of appended bodies of mass 1.0."""
    arrs = _crowd()
    cfg = make_cfg(theta=0.5)
    tr = outside_tracers(cfg, 256, 23)
    want_t, want_b = oracle_with_appended(arrs, cfg, tr, 3)
    eng = _engine(arrs, cfg, tr)
    eng.step(3)
    assert eng.num_bodies() < len(arrs[0]) - 260
    _assert_tracers(eng, want_t)
    _assert_bodies(eng, want_b)
    eng.close()


def test_replay_from_a_carried_tree():
    """The same after a merge-free pipelined call: the replayed call starts from the tree the
    previous call built ahead, and its snapshot is the caller-visible state."""
    arrs = _crowd()
    quiet = make_cfg(theta=0.5, merge_min_dist=0.0)
    cfg = make_cfg(theta=0.5)
    tr = outside_tracers(cfg, 256, 23)
    n = len(arrs[0])
    full = tuple(np.concatenate([a, t]) for a, t in zip(arrs, (*tr, np.ones(256))))
    ref = oracle.Oracle(*full, p=oracle.params(**quiet))
    ref.step(1)
    ref.set_params(oracle.params(**cfg))
    ref.step(3)
    out = ref.get_bodies()
    ref.close()
    nb = len(out[0]) - 256
    eng = _engine(arrs, quiet, tr)
    eng.step(1)
    assert eng.num_bodies() == n
    eng.set_params(params_of(cfg))
    eng.step(3)
    assert eng.num_bodies() == nb < n - 260
    _assert_tracers(eng, tuple(a[nb:] for a in out[:4]))
    _assert_bodies(eng, tuple(a[:nb] for a in out))
    eng.close()


def test_step_begin_end():
    cfg = make_cfg(theta=0.5)
    tr = tuple(a[:130] for a in _tracers())
    eng = bh_amd.Engine(params_of(cfg), device=0)
    eng.set_mirror(True, buffers=2)
    eng.reset_bodies(*_scene())
    eng.set_tracers(*tr)
    lib, h = eng._lib, eng._h
    view = bh_amd.default_view(width=64, height=48)
    own = np.empty((48, 64), dtype=np.uint32)
    buf = [np.empty(130) for _ in range(4)]
    got = ctypes.c_int64(0)
    eng.step_begin(2)
    rc_set = lib.bh_set_tracers(h, 130, *[a.ctypes.data_as(_D) for a in tr])
    rc_get = lib.bh_get_tracers(h, *[a.ctypes.data_as(_D) for a in buf], 130, ctypes.byref(got))
    rc_rnd = lib.bh_render_tracers(h, ctypes.byref(view), own.ctypes.data_as(_U32), None)
    eng.step_positions()
    eng.step_end()
    assert (rc_set, rc_get, rc_rnd) == (bh_amd.BH_E_STATE,) * 3
    want_t, want_b = _reference(0.5, 130, 2)
    _assert_tracers(eng, want_t)
    _assert_bodies(eng, want_b)
    eng.close()


def test_list_lifetime(tmp_path):
    cfg = make_cfg(theta=0.5)
    tr = tuple(a[:130] for a in _tracers())
    want1, _ = _reference(0.5, 130, 1)
    eng = _engine(_scene(), cfg, tr)
    with_tracers = str(tmp_path / "with.bhstate")
    eng.save_state(with_tracers)
    eng.step(0)
    _assert_tracers(eng, tr, "step(0) ")
    eng.step(1)
    _assert_tracers(eng, want1)
    # replaced mid-run by a longer list, then by a shorter one, then cleared
    eng.set_tracers(*(a[:300] for a in _tracers()))
    assert eng.num_tracers() == 300
    _assert_tracers(eng, tuple(a[:300] for a in _tracers()), "replaced ")
    eng.step(1)
    eng.set_tracers(tr[0][:7], tr[1][:7])  # vx, vy NULL: zeros
    got = eng.get_tracers()
    assert eng.num_tracers() == 7 and not got[2].any() and not np.signbit(got[2]).any()
    eng.step(1)
    eng.set_tracers(np.zeros(0), np.zeros(0))
    assert eng.num_tracers() == 0 and all(len(a) == 0 for a in eng.get_tracers())
    eng.step(1)
    # kept by reset_bodies, set_params and load_state; not written by save_state
    eng.set_tracers(*tr)
    eng.reset_bodies(*scenes.two_disks(60, 20))
    eng.set_params(params_of(make_cfg(theta=0.7)))
    _assert_tracers(eng, tr, "after reset ")
    eng.load_state(with_tracers)
    _assert_tracers(eng, tr, "after load ")
    eng.step(1)
    _assert_tracers(eng, want1, "resumed ")
    bare = _engine(_scene(), cfg)
    without = str(tmp_path / "without.bhstate")
    bare.save_state(without)
    assert open(with_tracers, "rb").read() == open(without, "rb").read()
    bare.close()
    # not touched by the queries and the renders
    before = eng.get_tracers()
    eng.compute_field(tr[0], tr[1])
    eng.compute_accelerations()
    eng.compute_potential()
    eng.get_quads()
    eng.render_bodies(width=64, height=48)
    eng.render_tracers(width=64, height=48)
    _assert_tracers(eng, before, "after queries ")
    eng.close()


def test_get_tracers_capacity_and_invalid_arguments():
    cfg = make_cfg(theta=0.5)
    tr = tuple(a[:65] for a in _tracers())
    eng = _engine(_scene(), cfg, tr)
    lib, h = eng._lib, eng._h
    got = ctypes.c_int64(0)
    small = np.full(10, 7.0)
    assert lib.bh_get_tracers(h, small.ctypes.data_as(_D), None, None, None, 10,
                              ctypes.byref(got)) == bh_amd.BH_E_CAPACITY
    assert got.value == 65 and (small == 7.0).all()
    for k in range(4):  # each plane alone, the others NULL
        out = np.empty(80)
        args = [None] * 4
        args[k] = out.ctypes.data_as(_D)
        got.value = 0
        assert lib.bh_get_tracers(h, *args, 80, ctypes.byref(got)) == bh_amd.BH_OK
        assert got.value == 65
        _assert_bits(out[:65], tr[k], TNAMES[k])
    assert lib.bh_get_tracers(h, None, None, None, None, 65, None) == bh_amd.BH_OK
    x, y = tr[0].ctypes.data_as(_D), tr[1].ctypes.data_as(_D)
    assert lib.bh_set_tracers(None, 65, x, y, None, None) == bh_amd.BH_E_INVALID
    assert lib.bh_get_tracers(None, None, None, None, None, 0, None) == bh_amd.BH_E_INVALID
    assert lib.bh_num_tracers(None) == -1
    for n, px, py in ((-1, x, y), ((1 << 28) + 1, x, y), (65, None, y), (65, x, None)):
        assert lib.bh_set_tracers(h, n, px, py, None, None) == bh_amd.BH_E_INVALID
        assert b"bh_set_tracers" in lib.bh_last_error(h)
    assert lib.bh_set_tracers(h, 0, None, None, None, None) == bh_amd.BH_OK  # n = 0: NULLs are fine
    assert eng.num_tracers() == 0
    out3 = (ctypes.c_int64 * 3)()
    assert lib.bh_tracer_launch_shape(10, None) == bh_amd.BH_E_INVALID
    assert lib.bh_tracer_launch_shape(-1, out3) == bh_amd.BH_E_INVALID
    ms = ctypes.c_double(0.0)
    assert lib.bh_tracer_kernel_ms(None, ctypes.byref(ms), None) == bh_amd.BH_E_INVALID
    assert lib.bh_tracer_kernel_ms(h, None, None) == bh_amd.BH_E_INVALID
    eng.close()


def _refused(eng, tr):
    with pytest.raises(bh_amd.BhError) as err:
        eng.set_tracers(*tr)
    assert err.value.rc == bh_amd.BH_E_STATE
    assert "locally essential" in str(err.value)
    eng.set_tracers(np.zeros(0), np.zeros(0))  # n = 0 is accepted everywhere
    assert eng.num_tracers() == 0


def test_refused_on_multi_rank_engines():
    cfg = make_cfg(theta=0.5)
    tr = tuple(a[:10] for a in _tracers())
    group = bh_amd.LocalGroup(2)
    members = [bh_amd.Engine(params_of(cfg), device=0, rank=r, local_group=group)
               for r in range(2)]
    _refused(members[0], tr)
    for m in members:
        m.close()
    group.close()
    multi = bh_amd.Engine(params_of(cfg), devices=[0, 0])
    assert multi.multi_world() == 2
    _refused(multi, tr)
    multi.reset_bodies(*scenes.two_disks(60, 20))  # (a small list: the handle's one-GPU engine)
    _refused(multi, tr)
    multi.close()


def _render_reference(tx, ty, view_x, view_y, zoom, width, height):
    """bh_render_bodies' pixel rule restated over a tracer list: drawn iff t is NaN or
    -1 < t < size, toInt (NaN -> 0, truncation), the later index wins."""
    with np.errstate(all="ignore"):
        u = (tx - view_x) * zoom
        v = (ty - view_y) * zoom
    nu, nv = np.isnan(u), np.isnan(v)
    drawn = (nu | ((u > -1.0) & (u < width))) & (nv | ((v > -1.0) & (v < height)))
    sx = np.where(nu, 0, np.trunc(np.where(drawn & ~nu, u, 0.0))).astype(np.int64)
    sy = np.where(nv, 0, np.trunc(np.where(drawn & ~nv, v, 0.0))).astype(np.int64)
    pix = (sy * width + sx)[drawn]
    idx = np.flatnonzero(drawn)
    owner = np.full(width * height, 0xFFFFFFFF, dtype=np.uint32)
    owner[pix] = idx  # ascending indices: the last assignment, the largest index, stays
    counts = np.bincount(pix, minlength=width * height).astype(np.uint32)
    return owner.reshape(height, width), counts.reshape(height, width)


@pytest.mark.parametrize("wh", [(64, 48), (2400, 800)])
def test_render_tracers(wh):
    width, height = wh
    cfg = make_cfg(theta=0.5)
    rng = np.random.default_rng(31)
    n = 5000
    vx0, vy0, zoom = 100.0, 50.0, width / 1200.0
    tx = rng.uniform(vx0 - 100.0, vx0 + 1300.0, n)  # (some left of, right of, above and below)
    ty = rng.uniform(vy0 - 50.0, vy0 + 1200.0 * height / width + 50.0, n)
    tx[:40] = vx0 - rng.uniform(0.0, 2.0, 40) / zoom   # up to two pixels left of the view
    ty[40:80] = vy0 - rng.uniform(0.0, 2.0, 40) / zoom  # ... and above it
    tx[80:90] = np.nan
    ty[85:95] = np.nan
    tx[95:200] = tx[300:405]  # several tracers on one pixel
    ty[95:200] = ty[300:405]
    eng = _engine(_scene(), cfg, (tx, ty))
    want_o, want_c = _render_reference(tx, ty, vx0, vy0, zoom, width, height)
    assert want_c.max() >= 2 and want_c[0, 0] >= 5 and (want_o == 0xFFFFFFFF).any()
    view = dict(view_x=vx0, view_y=vy0, zoom=zoom, width=width, height=height)
    own, cnt = eng.render_tracers(**view)
    assert np.array_equal(own, want_o) and np.array_equal(cnt, want_c)
    own, none = eng.render_tracers(counts=False, **view)  # each plane NULL in turn
    assert none is None and np.array_equal(own, want_o)
    none, cnt = eng.render_tracers(owner=False, **view)
    assert none is None and np.array_equal(cnt, want_c)
    # the body pass is unchanged beside it, and the tracers are as they were
    pix = eng.render_bodies(width=width, height=height)
    bare = _engine(_scene(), cfg)
    assert np.array_equal(pix, bare.render_bodies(width=width, height=height))
    bare.close()
    _assert_tracers(eng, (tx, ty, np.zeros(n), np.zeros(n)), nan_equal=True)
    # no tracers: all-empty planes
    eng.set_tracers(np.zeros(0), np.zeros(0))
    own, cnt = eng.render_tracers(**view)
    assert (own == 0xFFFFFFFF).all() and not cnt.any()
    # the view is checked as bh_render_bodies checks it, with its text
    for bad in (dict(zoom=0.0), dict(width=0), dict(height=20000)):
        errs = []
        for fn in (eng.render_tracers, eng.render_bodies):
            with pytest.raises(bh_amd.BhError) as err:
                fn(**{**view, **bad})
            assert err.value.rc == bh_amd.BH_E_INVALID
            errs.append(str(err.value))
        assert errs[0] == errs[1]
    eng.close()


def test_tracer_kernel_ms():
    cfg = make_cfg(theta=0.5)
    eng = _engine(_scene(), cfg, tuple(a[:130] for a in _tracers()))
    eng.step(2)
    assert eng.tracer_kernel_ms() == (0.0, 0)  # no events unless profiling is on
    eng.set_profiling(True)
    k = 3
    eng.step(k)
    ms, launches = eng.tracer_kernel_ms()
    assert launches == 2 * k and 0.0 < ms < 1000.0
    # the traversals are counted as an engine without tracers counts them (a call that starts on
    # a carried tree has no event before its first traversal)
    bare = _engine(_scene(), cfg)
    bare.step(2)
    bare.set_profiling(True)
    bare.step(k)
    assert eng.traverse_kernel_ms()[1] == bare.traverse_kernel_ms()[1] >= 2 * k - 1
    assert bare.tracer_kernel_ms() == (0.0, 0)
    bare.close()
    assert eng.last_timings()["traverse"] >= ms * launches * 0.999  # the walks are under phase [1]
    eng.set_profiling(False)
    eng.step(1)
    assert eng.tracer_kernel_ms() == (0.0, 0)
    # without tracers nothing is launched
    eng.set_tracers(np.zeros(0), np.zeros(0))
    eng.set_profiling(True)
    eng.step(1)
    assert eng.tracer_kernel_ms() == (0.0, 0)
    want_b = _oracle_bodies(_scene(), cfg, 2 + k + 2)
    _assert_bodies(eng, want_b)
    eng.close()
