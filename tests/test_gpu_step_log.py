"""GPU: the step log (bh_set_step_log) -- one conservation record per step, made inside bh_step
from the step's own second traversal -- against the existing read-out on a twin engine (bit for
bit, on steps that neither jitter nor merge) and against the Python reference of
tests/test_step_log_ref.py (phi bit for bit, the sums within the summation bound)."""
import ctypes
import functools
import math
import struct

import numpy as np
import pytest

import bh_amd
import oracle
import test_launch_plan as lp
from bh_amd import scenes
from test_gpu_tracers import _crowd
from test_oracle import massless_cells_scene, with_far_bodies, with_heavy_body
from test_potential_ref import make_cfg, params_of, sum_bound, theta0_phi
from test_step_log_ref import (FIELDS, SUMS, build_moves_nothing, golden_start, record_terms,
                               reference_log)

pytestmark = pytest.mark.gpu

_D = ctypes.POINTER(ctypes.c_double)


def _engine(arrs, cfg, log=16, **kw):
    eng = bh_amd.Engine(params_of(cfg), **({"device": 0} if not kw else kw))
    eng.reset_bodies(*arrs)
    if log:
        eng.set_step_log(log)
    return eng


def _bits(v):
    return struct.pack("<d", float(v))


def _assert_bits(got, want, what, nan_equal=False):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    diff = got.view(np.int64) != want.view(np.int64)
    if nan_equal:  # (a NaN's sign and payload are not the reference's to define)
        diff &= ~(np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(diff)
    assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {bad[:5]}: "
                           f"{got[bad[:3]]} vs {want[bad[:3]]}")


def _assert_diag_bits(got, want, what):
    assert got.n == want.n, f"{what}: n {got.n} vs {want.n}"
    for f in SUMS:
        assert _bits(getattr(got, f)) == _bits(getattr(want, f)), \
            f"{what}: {f} {getattr(got, f)!r} vs {getattr(want, f)!r}"


def _assert_logs_equal(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} vs {len(b)} records"
    for ra, rb in zip(a, b):
        assert ra.step == rb.step and _bits(ra.t) == _bits(rb.t), f"{what}: step {ra.step}"
        _assert_diag_bits(ra.d, rb.d, f"{what}: record {ra.step}")


def _moves_nothing(state, cfg):
    """A build of `state` jitters no body: the Python oracle's build, or from 20 000 bodies up
    the C oracle's (the same buildTree, BHA:359-366, in a fraction of the time)."""
    if len(state[0]) <= 20_000:
        return build_moves_nothing(state, cfg)
    ref = oracle.Oracle(*state, p=oracle.params(**cfg))
    ref.accelerations(subset=np.zeros(1, dtype=np.int64))
    after = ref.get_bodies()
    ref.close()
    return (np.array_equal(after[0].view(np.int64), np.asarray(state[0]).view(np.int64)) and
            np.array_equal(after[1].view(np.int64), np.asarray(state[1]).view(np.int64)))


def _twin_check(arrs, cfg, k, phi_reference=None):
    """Engine A logs k steps in one call; twin B makes k one-step calls with the existing
    read-out after each.  No build of B's states moves a body (asserted), so the records must be
    B's results bit for bit, and the last step's phi B's compute_potential."""
    a, b = _engine(arrs, cfg), _engine(arrs, cfg, log=0)
    try:
        a.step(k)
        log = a.get_step_log()
        assert [r.step for r in log] == list(range(1, k + 1))
        t = 0.0
        for s in range(k):
            b.step(1)
            state = b.get_bodies()
            assert _moves_nothing(state, cfg), f"step {s + 1}: the scene jitters"
            d = b.diagnostics(potential=True)
            t += cfg["dt"]
            assert _bits(log[s].t) == _bits(t)
            _assert_diag_bits(log[s].d, d, f"record {s + 1}")
        assert b.num_bodies() == len(arrs[0])  # nothing merged
        phi = a.get_step_log_phi()
        _assert_bits(phi, b.compute_potential(), "phi of the last step")
        if phi_reference is not None:
            want, _ = phi_reference(state, cfg)
            _assert_bits(phi, want, "phi against the reference")
    finally:
        a.close()
        b.close()


# ---- 1. bit-equality with the existing read-out ------------------------------------------------

QUIET = dict(merge_min_dist=0.0)


@pytest.mark.parametrize("theta", [0.2, 0.5, 1.0])
def test_records_equal_the_twins_diagnostics(theta):
    _twin_check(scenes.two_disks(1500, 500), make_cfg(theta=theta, **QUIET), 5)


def test_full_waves_eight_per_workgroup():
    arrs = scenes.kepler_disk(66_000)
    plan = lp.plan(66_000)
    assert (plan["kick_bpw"], plan["kick_wpb"]) == (64, 8)
    _twin_check(arrs, make_cfg(theta=0.5, **QUIET), 3)


def _kick_shape_sizes():
    cuts = set(lp.field_boundaries("kick_bpw", 2, 600_000))
    cuts |= set(lp.field_boundaries("kick_wpb", 2, 600_000))
    return sorted(s for b in cuts for s in (b - 1, b))


@pytest.mark.parametrize("n", _kick_shape_sizes())
def test_kick_walk_launch_shapes(n):
    """b - 1 and b wherever the plan changes the kick-only walk's bodies per wave or waves per
    workgroup (the sizes are read from bh_launch_plan, none is written down)."""
    _twin_check(scenes.uniform(n, 1.0, seed=31), make_cfg(theta=0.5, **QUIET), 2)


def test_lane_map_resort_inside_the_call():
    _twin_check(scenes.two_disks(1500, 500), make_cfg(theta=0.5, **QUIET), 10)


# ---- 2. against the Python reference -------------------------------------------------------

def _reference_check(arrs, cfg, calls, nan_at=None):
    """phi after every call bit for bit, every record's n exactly and its sums within the bound
    of any-order fp64 summation around the exactly rounded sums of the reference's terms.
    nan_at: the bodies whose phi is NaN in the reference (none: every phi is finite); a sum with a
    NaN term is NaN."""
    k = sum(calls)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        want, pe = reference_log(arrs, cfg, k)
    eng = _engine(arrs, cfg)
    try:
        done = 0
        for c in calls:
            eng.step(c)
            done += c
            odd = np.flatnonzero(~np.isfinite(want[done - 1]["phi"]))
            assert np.array_equal(odd, [] if nan_at is None else nan_at), \
                "the reference's phi is not finite"
            assert np.all(np.isnan(want[done - 1]["phi"][odd]))
            _assert_bits(eng.get_step_log_phi(), want[done - 1]["phi"], f"phi of step {done}",
                         nan_equal=nan_at is not None)
        log = eng.get_step_log()
        assert len(log) == k
        t = 0.0
        for s, (rec, ref) in enumerate(zip(log, want)):
            t += cfg["dt"]
            assert rec.step == s + 1 == ref["step"] and _bits(rec.t) == _bits(t) == _bits(ref["t"])
            assert rec.d.n == ref["n"], f"record {s + 1}: n"
            for name, terms in record_terms(ref).items():
                exact, bound = math.fsum(terms.tolist()), sum_bound(terms)
                if name == "potential":
                    exact, bound = 0.5 * exact, 0.5 * bound
                got = getattr(rec.d, name)
                print(f"step {s + 1} {name}: got {got!r} want {exact!r} "
                      f"|diff| {abs(got - exact):.3e} bound {bound:.3e}")
                if math.isnan(exact):
                    assert nan_at is not None and math.isnan(got), (s + 1, name)
                else:
                    assert abs(got - exact) <= bound, (s + 1, name)
        assert eng.num_bodies() == len(pe.bodies)
        return log, want
    finally:
        eng.close()


@pytest.mark.parametrize("n", [1, 2, 63, 65, 130])
def test_small_sizes(n):
    arrs = tuple(a[:n].copy() for a in scenes.two_disks(100, 40))
    log, _ = _reference_check(arrs, make_cfg(theta=0.5), (1, 1))
    if n == 1:
        assert all(r.d.potential == 0.0 for r in log)


@pytest.mark.parametrize("name,calls", [("merge_127.npz", (4, 2)), ("jitter_306.npz", (1, 2)),
                                        ("outside_153.npz", (2,))])
def test_goldens(name, calls):
    arrs, cfg = golden_start(name)
    log, want = _reference_check(arrs, cfg, calls)
    if name.startswith("merge"):  # removals inside the first call
        ns = [r.d.n for r in log]
        assert ns[0] == len(arrs[0]) and ns[3] < ns[0]


def test_zero_mass_bodies():
    arrs = tuple(a.copy() for a in scenes.two_disks(600, 200))
    zero = np.sort(np.random.default_rng(3).choice(800, 20, replace=False))
    arrs[4][zero] = 0.0
    # F / m = 0 / 0 (BHA:390-391): the first kick makes the massless bodies' velocities and
    # positions NaN; they fall out of the tree, their walk opens every node and phi is NaN
    _reference_check(arrs, make_cfg(theta=0.5), (2,), nan_at=zero)


def test_negative_mass_cells():
    """NODE_SKIP on the exact walk (soft2 = 0 sends every wave there): massless cells of
    negative-mass bodies are not visited, and with soft2 = 0 a visit would show as 0 * inf."""
    _reference_check(massless_cells_scene(1200), make_cfg(theta=0.5, soft2=0.0), (2,))


# ---- 3. grouping -----------------------------------------------------------------------------

def test_grouping_of_steps_into_calls():
    arrs, cfg = golden_start("merge_127.npz")
    logs = []
    for calls in ((6,), (1,) * 6, (2, 4)):
        eng = _engine(arrs, cfg)
        for c in calls:
            eng.step(c)
        logs.append((eng.get_step_log(), eng.get_step_log_phi(), eng.num_bodies()))
        eng.close()
    for other in logs[1:]:
        _assert_logs_equal(logs[0][0], other[0], "grouping")
        _assert_bits(logs[0][1], other[1], "phi of the last step")
    ns = [r.d.n for r in logs[0][0]]
    assert ns[0] == len(arrs[0]) and ns == sorted(ns, reverse=True) and ns[-1] < ns[0]
    assert logs[0][2] <= ns[-1]


# ---- 4. theta = 0 ------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", [(800, 224), (1600, 500)])
def test_theta0(n1, n2):
    """The unpipelined step: the all-pairs potential over the evaluation's leaf list (1024 leaves
    fill one tile exactly, 2100 cross two)."""
    _twin_check(scenes.two_disks(n1, n2), make_cfg(theta=0.0, **QUIET), 2,
                phi_reference=theta0_phi)


# ---- 5. IEEE paths ---------------------------------------------------------------------------

def _ieee_case(case, arrs):
    cfg = make_cfg(theta=0.5, **QUIET)
    if case == "soft2_0":
        cfg["soft2"] = 0.0
    elif case == "far":
        arrs = with_far_bodies(arrs)
        assert abs(arrs[0][0]) == 1e100
    else:  # G m^2 beyond lane_self_ok's 2^400
        arrs = with_heavy_body(arrs, 1e61, min(1234, len(arrs[0]) - 1))
    return arrs, cfg


@pytest.mark.parametrize("case", ["soft2_0", "far", "heavy"])
def test_ieee_paths_against_the_twin(case):
    arrs, cfg = _ieee_case(case, scenes.two_disks(2500, 700))
    a, b = _engine(arrs, cfg), _engine(arrs, cfg, log=0)
    try:
        a.step(1)
        b.step(1)
        assert build_moves_nothing(b.get_bodies(), cfg)
        phi = a.get_step_log_phi()
        assert np.all(np.isfinite(phi))
        _assert_bits(phi, b.compute_potential(), "phi")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("case", ["soft2_0", "far", "heavy"])
def test_ieee_paths_against_the_reference(case):
    cut = tuple(a[:300].copy() for a in scenes.two_disks(2500, 700))
    arrs, cfg = _ieee_case(case, cut)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        want, _ = reference_log(arrs, cfg, 1)
    assert np.all(np.isfinite(want[0]["phi"]))
    eng = _engine(arrs, cfg)
    try:
        eng.step(1)
        _assert_bits(eng.get_step_log_phi(), want[0]["phi"], "phi")
        assert eng.get_step_log()[0].d.n == len(arrs[0])
    finally:
        eng.close()


# ---- 6. replay -------------------------------------------------------------------------------

@pytest.mark.parametrize("carried", [False, True])
def test_replayed_call_logs_each_step_once(carried):
    """The first step's candidate pairs overflow the merge mailbox and the call is replayed:
    exactly records 1 and 2 (after a merge-free pipelined call: 2 and 3), the first with the
    initial N, bit-identical to two one-step calls."""
    arrs = _crowd()
    quiet, cfg = make_cfg(theta=0.5, **QUIET), make_cfg(theta=0.5)
    logs = []
    for calls in ((2,), (1, 1)):
        eng = _engine(arrs, quiet if carried else cfg)
        if carried:
            eng.step(1)
            eng.set_params(params_of(cfg))
        for c in calls:
            eng.step(c)
        logs.append(eng.get_step_log())
        assert eng.num_bodies() < len(arrs[0]) - 260
        eng.close()
    first = 1 if carried else 0
    assert [r.step for r in logs[0]] == list(range(1, first + 3))
    assert logs[0][first].d.n == len(arrs[0]) > logs[0][first + 1].d.n
    _assert_logs_equal(logs[0], logs[1], "replayed call")


# ---- 7. ring and life cycle --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scene():
    return scenes.two_disks(300, 100)


def test_ring_overwrites_its_oldest_record():
    cfg = make_cfg(theta=0.5)
    ring, twin = _engine(_scene(), cfg, log=4), _engine(_scene(), cfg, log=16)
    for eng in (ring, twin):
        eng.step(3)
        eng.step(3)
    got, want = ring.get_step_log(), twin.get_step_log()
    assert [r.step for r in got] == [3, 4, 5, 6] and len(want) == 6
    _assert_logs_equal(got, want[2:], "ring")
    _assert_bits(ring.get_step_log_phi(), twin.get_step_log_phi(), "phi")
    ring.set_step_log(4)  # re-setting the capacity empties the log
    assert ring.get_step_log() == []
    with pytest.raises(bh_amd.BhError) as err:
        ring.get_step_log_phi()
    assert err.value.rc == bh_amd.BH_E_STATE
    ring.step(1)
    assert [(r.step, r.t) for r in ring.get_step_log()] == [(1, cfg["dt"])]
    ring.set_step_log(0)  # off: buffers freed, the getters return nothing
    assert ring.get_step_log() == [] and len(ring.get_step_log_phi()) == 0
    ring.step(1)
    assert ring.get_step_log() == []
    ring.close()
    twin.close()


def test_log_persists_across_reset_params_and_load(tmp_path):
    cfg = make_cfg(theta=0.5, **QUIET)
    eng = _engine(_scene(), cfg)
    path = str(tmp_path / "s.bhstate")
    eng.save_state(path)
    eng.step(0)
    assert eng.get_step_log() == []
    eng.step(2)
    eng.reset_bodies(*scenes.two_disks(60, 20))
    assert [r.step for r in eng.get_step_log()] == [1, 2]
    with pytest.raises(bh_amd.BhError) as err:  # no step logged since the bodies were replaced
        eng.get_step_log_phi()
    assert err.value.rc == bh_amd.BH_E_STATE
    eng.set_params(params_of(make_cfg(theta=0.5, dt=0.25, **QUIET)))  # dt is read per call
    eng.step(1)
    eng.load_state(path)  # (brings the saved dt back)
    with pytest.raises(bh_amd.BhError):
        eng.get_step_log_phi()
    eng.step(1)
    log = eng.get_step_log()
    assert [r.step for r in log] == [1, 2, 3, 4] and [r.d.n for r in log] == [400, 400, 80, 400]
    t = [0.0 + cfg["dt"]]
    for dt in (cfg["dt"], 0.25, cfg["dt"]):
        t.append(t[-1] + dt)
    assert [_bits(r.t) for r in log] == [_bits(v) for v in t]
    fresh = _engine(_scene(), cfg)  # the resumed step is the saved state's first
    fresh.step(1)
    _assert_diag_bits(log[3].d, fresh.get_step_log()[0].d, "resumed")
    _assert_bits(eng.get_step_log_phi(), fresh.get_step_log_phi(), "phi")
    bare = _engine(_scene(), cfg, log=0)  # the log is not written by save_state
    other = str(tmp_path / "bare.bhstate")
    bare.save_state(other)
    assert open(path, "rb").read() == open(other, "rb").read()
    for e in (eng, fresh, bare):
        e.close()


def test_capacity_and_invalid_arguments():
    eng = _engine(_scene(), make_cfg(theta=0.5, **QUIET), log=8)
    eng.step(3)
    lib, h = eng._lib, eng._h
    n = ctypes.c_int64(0)
    recs = (bh_amd.BhStepRecord * 8)()
    recs[0].step = 77
    assert lib.bh_get_step_log(h, recs, 2, ctypes.byref(n)) == bh_amd.BH_E_CAPACITY
    assert n.value == 3 and recs[0].step == 77
    assert lib.bh_get_step_log(h, recs, 8, ctypes.byref(n)) == bh_amd.BH_OK
    assert n.value == 3 and [recs[i].step for i in range(3)] == [1, 2, 3]
    phi = np.full(400, 7.0)
    assert lib.bh_get_step_log_phi(h, phi.ctypes.data_as(_D), 399,
                                   ctypes.byref(n)) == bh_amd.BH_E_CAPACITY
    assert n.value == 400 and (phi == 7.0).all()
    assert lib.bh_get_step_log_phi(h, phi.ctypes.data_as(_D), 400, ctypes.byref(n)) == bh_amd.BH_OK
    assert (phi < 0.0).all()
    for rc in (lib.bh_set_step_log(None, 4), lib.bh_set_step_log(h, -1),
               lib.bh_set_step_log(h, (1 << 20) + 1),
               lib.bh_get_step_log(None, recs, 8, ctypes.byref(n)),
               lib.bh_get_step_log(h, recs, 8, None),
               lib.bh_get_step_log(h, None, 8, ctypes.byref(n)),
               lib.bh_get_step_log_phi(None, phi.ctypes.data_as(_D), 400, ctypes.byref(n)),
               lib.bh_get_step_log_phi(h, phi.ctypes.data_as(_D), 400, None),
               lib.bh_get_step_log_phi(h, None, 400, ctypes.byref(n)),
               lib.bh_step_log_kernel_ms(None, ctypes.byref(ctypes.c_double()), None),
               lib.bh_step_log_kernel_ms(h, None, None)):
        assert rc == bh_amd.BH_E_INVALID
    assert len(eng.get_step_log()) == 3  # the refused calls changed nothing
    assert eng.step_log_kernel_ms() == (0.0, 0)  # only while profiling
    eng.set_profiling(True)
    eng.step(2)
    ms, launches = eng.step_log_kernel_ms()
    assert launches == 2 and ms > 0.0
    eng.close()


def _refused(eng):
    with pytest.raises(bh_amd.BhError) as err:
        eng.set_step_log(8)
    assert err.value.rc == bh_amd.BH_E_STATE
    assert "locally essential" in str(err.value)
    eng.set_step_log(0)  # capacity 0 is accepted everywhere
    assert eng.get_step_log() == []


def test_refused_on_multi_rank_engines():
    cfg = make_cfg(theta=0.5)
    group = bh_amd.LocalGroup(2)
    members = [bh_amd.Engine(params_of(cfg), device=0, rank=r, local_group=group)
               for r in range(2)]
    _refused(members[0])
    for m in members:
        m.close()
    group.close()
    multi = bh_amd.Engine(params_of(cfg), devices=[0, 0])
    assert multi.multi_world() == 2
    _refused(multi)
    multi.reset_bodies(*scenes.two_disks(60, 20))  # (a small list: the handle's one-GPU engine)
    _refused(multi)
    multi.close()


def test_step_begin_end():
    cfg = make_cfg(theta=0.5)
    eng = bh_amd.Engine(params_of(cfg), device=0)
    eng.set_mirror(True, buffers=2)
    eng.reset_bodies(*_scene())
    eng.set_step_log(8)
    lib, h = eng._lib, eng._h
    n = ctypes.c_int64(0)
    recs = (bh_amd.BhStepRecord * 8)()
    phi = np.empty(400)
    eng.step_begin(2)
    rcs = (lib.bh_set_step_log(h, 4), lib.bh_get_step_log(h, recs, 8, ctypes.byref(n)),
           lib.bh_get_step_log_phi(h, phi.ctypes.data_as(_D), 400, ctypes.byref(n)))
    eng.step_positions()
    eng.step_end()
    assert rcs == (bh_amd.BH_E_STATE,) * 3
    sync = _engine(_scene(), cfg, log=8)
    sync.step(2)
    _assert_logs_equal(eng.get_step_log(), sync.get_step_log(), "step_begin / step_end")
    _assert_bits(eng.get_step_log_phi(), sync.get_step_log_phi(), "phi")
    eng.close()
    sync.close()


def test_failed_call_empties_the_ring():
    cfg = make_cfg(theta=0.5)
    eng = _engine(_scene(), cfg)
    eng.step(2)
    before = eng.get_step_log()
    eng.debug_inject(2)  # the next full build raises its tree flag
    with pytest.raises(bh_amd.BhError) as err:
        eng.step(2)
    assert err.value.rc == bh_amd.BH_E_STATE
    assert eng.get_step_log() == []
    with pytest.raises(bh_amd.BhError):
        eng.get_step_log_phi()
    eng.reset_bodies(*_scene())
    eng.step(1)
    log = eng.get_step_log()  # step and t go on from their values before the failed call
    assert [r.step for r in log] == [3]
    assert _bits(log[0].t) == _bits(before[1].t + cfg["dt"])
    eng.close()


# ---- 8. no effect on the simulation ------------------------------------------------------------

@pytest.mark.parametrize("scene", ["c1_baseline", "merge_127"])
def test_log_changes_nothing_else(scene):
    if scene == "c1_baseline":
        arrs, cfg = scenes.config_scene("c1_baseline"), make_cfg(theta=0.5)
    else:
        arrs, cfg = golden_start("merge_127.npz")
    tr = tuple(a[:130].copy() for a in scenes.two_disks(100, 40)[:4])
    plain = _engine(arrs, cfg, log=0)
    plain.set_tracers(*tr)
    plain.step(5)
    want = plain.get_bodies(), plain.last_removed(), plain.get_tracers()
    logs = []
    for mirror in (0, 1, 2):
        eng = bh_amd.Engine(params_of(cfg), device=0)
        if mirror:
            eng.set_mirror(True, buffers=mirror)
        eng.reset_bodies(*arrs)
        eng.set_tracers(*tr)
        eng.set_step_log(16)
        eng.step(5)
        for name, g, w in zip(FIELDS, eng.get_bodies(), want[0]):
            _assert_bits(g, w, f"mirror {mirror}: {name}")
        assert np.array_equal(eng.last_removed(), want[1])
        for g, w in zip(eng.get_tracers(), want[2]):
            _assert_bits(g, w, f"mirror {mirror}: tracers")
        logs.append(eng.get_step_log())
        eng.close()
    plain.close()
    for other in logs[1:]:  # ... and the mirror does not change the records
        _assert_logs_equal(logs[0], other, "mirror")
    bare = _engine(arrs, cfg)  # nor do the tracers
    bare.step(5)
    _assert_logs_equal(logs[0], bare.get_step_log(), "tracers")
    bare.close()


def test_no_bodies():
    empty = tuple(np.zeros(0) for _ in range(5))
    cfg = make_cfg(theta=0.5)
    eng = _engine(empty, cfg)
    eng.step(3)
    log = eng.get_step_log()
    zero = bh_amd.Diagnostics(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    t = [cfg["dt"], cfg["dt"] + cfg["dt"], cfg["dt"] + cfg["dt"] + cfg["dt"]]
    assert [(r.step, _bits(r.t)) for r in log] == [(s + 1, _bits(t[s])) for s in range(3)]
    for r in log:
        _assert_diag_bits(r.d, zero, "N = 0")
    assert len(eng.get_step_log_phi()) == 0
    eng.close()
