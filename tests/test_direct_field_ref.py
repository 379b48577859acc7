"""bh_compute_field_direct / bh_compute_force_error on CPU: the boundary, the launch-shape
read-out, the summary's restatement and the pinned reference of the exact accelerations.

`force_error_summary(ax_t, ay_t, ax_e, ay_e)` restates the summary of bh_compute_force_error
(include/bh_engine.h) with sequential loops on Python floats (binary64, nothing fused);
tests/test_gpu_direct_field.py checks the engine's summary bit for bit against it.
"""
import ctypes
import math
import os
import re

import numpy as np

import bh_amd
import oracle
from test_field_ref import FIELDS, GOLDEN, HEADER, checker_field, root_cell
from test_potential_ref import cfg_from_golden

_I64P = ctypes.POINTER(ctypes.c_int64)
_D = ctypes.POINTER(ctypes.c_double)

NEW_FUNCTIONS = ("bh_compute_field_direct", "bh_compute_force_error", "bh_direct_field_kernel_ms",
                 "bh_direct_field_shape")
# The documented launch-shape choice (DESIGN "Exact field and force error", bh_engine.h): one-wave
# workgroups around a 256-leaf tile up to SMALL_MAX targets, k_direct's shape above.
SMALL_MAX = 32768
SMALL_SHAPE = (256, 64, 1)
LARGE_SHAPE = (1024, 256, 2)


def force_error_summary(ax_t, ay_t, ax_e, ay_e):
    """dict(n_sample, n_used, worst, max_rel, mean_rel, rms_rel) of the four sample arrays."""
    k = len(ax_t)
    n_used, worst = 0, -1
    max_rel = total = total_sq = 0.0
    for j in range(k):
        at = (float(ax_t[j]), float(ay_t[j]))
        ex, ey = float(ax_e[j]), float(ay_e[j])
        if not all(math.isfinite(v) for v in (*at, ex, ey)):
            continue
        den = math.sqrt(ex * ex + ey * ey)
        if not den > 0.0:
            continue
        dx = at[0] - ex
        dy = at[1] - ey
        rel = math.sqrt(dx * dx + dy * dy) / den  # (den > 0: no exception; inf / inf is NaN)
        if n_used == 0 or rel > max_rel:  # the first on ties
            max_rel, worst = rel, j
        total += rel
        total_sq += rel * rel
        n_used += 1
    mean_rel = total / n_used if n_used else 0.0
    rms_rel = math.sqrt(total_sq / n_used) if n_used else 0.0
    return dict(n_sample=k, n_used=n_used, worst=worst, max_rel=max_rel, mean_rel=mean_rel,
                rms_rel=rms_rel)


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def test_header_declares_the_new_calls():
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert name in bh_amd.EXPORTED_SYMBOLS
    m = re.search(r"typedef\s+struct\s+bh_force_error\s*\{(.*?)\}\s*bh_force_error\s*;", code,
                  flags=re.S)
    assert m, "struct bh_force_error not declared"
    fields = re.findall(r"\b(n_sample|n_used|worst|max_rel|mean_rel|rms_rel)\b", m.group(1))
    assert fields == ["n_sample", "n_used", "worst", "max_rel", "mean_rel", "rms_rel"]
    assert [f for f, _ in bh_amd.BhForceError._fields_] == fields
    assert ctypes.sizeof(bh_amd.BhForceError) == 48
    # both calls are in the list of calls refused between bh_step_begin and bh_step_end
    guard = txt[txt.index("bh_step(e, k) on a thread"):txt.index("int bh_step_begin")]
    assert "bh_compute_field_direct" in guard and "bh_compute_force_error" in guard
    # bh_compute_field's own comment points to the new call
    field_doc = txt[txt.index("The field of the current state"):txt.index("int bh_compute_field(")]
    assert "bh_compute_field_direct" in field_doc


def test_shape_read_out(engine_lib):
    """Host-only, no device: the values come from the function the launch branches on."""
    out = np.zeros(3, dtype=np.int64)
    for n in (0, 1, 63, 64, 65, 4096, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 120_000, 10 ** 6,
              1 << 28):
        assert engine_lib.bh_direct_field_shape(n, out.ctypes.data_as(_I64P)) == bh_amd.BH_OK
        tile, lanes, per_lane = (int(v) for v in out)
        assert tile >= 64 and lanes % 64 == 0 and lanes >= 64 and per_lane >= 1
        assert tile % lanes == 0  # whole staging passes
        assert (tile, lanes, per_lane) == bh_amd.direct_field_shape(n)
        assert (tile, lanes, per_lane) == (SMALL_SHAPE if n <= SMALL_MAX else LARGE_SHAPE), n
    assert bh_amd.direct_field_shape(1) == SMALL_SHAPE
    # 4096 targets are 64 one-wave workgroups, not 16 workgroups of 256
    tile, lanes, per_lane = bh_amd.direct_field_shape(4096)
    assert lanes == 64 and 4096 // (lanes * per_lane) == 64
    assert bh_amd.direct_field_shape(10 ** 6) == LARGE_SHAPE
    assert engine_lib.bh_direct_field_shape(10, None) == bh_amd.BH_E_INVALID
    assert engine_lib.bh_direct_field_shape(-1, out.ctypes.data_as(_I64P)) == bh_amd.BH_E_INVALID


def test_null_engine_is_invalid(engine_lib):
    p = np.zeros(4)
    dp = p.ctypes.data_as(_D)
    idx = np.zeros(4, dtype=np.int64)
    assert engine_lib.bh_compute_field_direct(None, 4, dp, dp, None, None, None,
                                              None) == bh_amd.BH_E_INVALID
    assert engine_lib.bh_compute_force_error(None, 4, idx.ctypes.data_as(_I64P), None, None, None,
                                             None, None) == bh_amd.BH_E_INVALID
    ms = ctypes.c_double(1.0)
    assert engine_lib.bh_direct_field_kernel_ms(None, ctypes.byref(ms)) == bh_amd.BH_E_INVALID


def test_summary_hand_made_cases():
    a = np.array([1.0, -2.0, 3.0, 0.5])
    b = np.array([0.0, 4.0, -1.0, 2.0])
    s = force_error_summary(a, b, a, b)  # all equal: zeros, worst = the first used
    assert s == dict(n_sample=4, n_used=4, worst=0, max_rel=0.0, mean_rel=0.0, rms_rel=0.0)
    # sample 0 has a NaN, sample 1 a zero denominator: worst = the first used, sample 2
    ax_e, ay_e = a.copy(), b.copy()
    ax_t, ay_t = a.copy(), b.copy()
    ax_t[0] = math.nan
    ax_e[1] = ay_e[1] = 0.0
    s = force_error_summary(ax_t, ay_t, ax_e, ay_e)
    assert (s["n_used"], s["worst"], s["max_rel"]) == (2, 2, 0.0)
    ax_e[0] = math.inf  # a non-finite exact value excludes the sample too
    ax_t[0] = 1.0
    assert force_error_summary(ax_t, ay_t, ax_e, ay_e)["n_used"] == 2
    # known values: exact (3, 4), tree off by (0.3, 0.4) -> 0.5 / 5; and by (0, 0.05) -> 0.01
    ax_e, ay_e = np.array([3.0, 3.0, 3.0]), np.array([4.0, 4.0, 4.0])
    ax_t, ay_t = np.array([3.0, 3.3, 3.3]), np.array([4.05, 4.4, 4.4])
    s = force_error_summary(ax_t, ay_t, ax_e, ay_e)
    r0 = math.sqrt(0.0 * 0.0 + (4.05 - 4.0) * (4.05 - 4.0)) / 5.0
    r1 = math.sqrt((3.3 - 3.0) * (3.3 - 3.0) + (4.4 - 4.0) * (4.4 - 4.0)) / 5.0
    assert s["worst"] == 1 and s["max_rel"] == r1  # ties: the first
    assert s["mean_rel"] == (r0 + r1 + r1) / 3
    assert s["rms_rel"] == math.sqrt((r0 * r0 + r1 * r1 + r1 * r1) / 3)
    assert math.isclose(r1, 0.1, rel_tol=1e-12) and math.isclose(r0, 0.01, rel_tol=1e-12)
    # nothing usable, and nothing at all
    s = force_error_summary([math.nan], [1.0], [1.0], [1.0])
    assert s == dict(n_sample=1, n_used=0, worst=-1, max_rel=0.0, mean_rel=0.0, rms_rel=0.0)
    assert force_error_summary([], [], [], [])["worst"] == -1


def test_exact_acceleration_reference_is_pinned():
    """a_exact's reference: the C oracle's accelerations() at theta = 0 equals, bit for bit, the
    field checker at theta = 0 at every in-tree body's jittered position with its mass -- the
    probe takes the body's own leaf too, whose force term is an exact zero because soft2 > 0."""
    z = np.load(os.path.join(GOLDEN, "two_disks_600_theta0.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    assert cfg["theta"] == 0.0 and cfg["soft2"] > 0.0
    ref = oracle.Oracle(*arrs, p=oracle.params(**cfg))
    oax, oay = ref.accelerations()
    st = ref.get_bodies()  # after the build: the jitter is in
    ref.close()
    cx, cy, h = root_cell(cfg)
    inside = np.flatnonzero((st[0] >= cx - h) & (st[0] < cx + h) & (st[1] >= cy - h) &
                            (st[1] < cy + h))
    assert inside.size == len(st[0]) == 600  # the scene: every body is in the tree
    assert np.all(st[4] != 0.0)
    ax, ay, _, cst = checker_field(arrs, cfg, st[0][inside], st[1][inside], st[4][inside])
    for name, a, b in zip(FIELDS, cst, st):
        assert np.array_equal(_bits(a), _bits(b)), name  # the checker's tree is the oracle's
    assert np.array_equal(_bits(ax), _bits(oax[inside]))
    assert np.array_equal(_bits(ay), _bits(oay[inside]))
