"""GPU: what the read-only queries share -- the kernel stopwatches, the refusal texts of the
count-and-pointer checks, and buffers that are kept when a later call asks for less.

Nothing here depends on a value of the field: the value checks are bit comparisons against the same
call on a fresh engine that was given the same body list.
"""
import ctypes
import math

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes

pytestmark = pytest.mark.gpu

_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)
FIELDS = ("x", "y", "vx", "vy", "m")
TOO_MANY = (1 << 28) + 1


def _three():
    """Three bodies, apart from each other and inside the default 2400 x 800 world."""
    return (np.array([700.0, 1300.0, 1900.0]), np.array([300.0, 500.0, 200.0]),
            np.array([1.0, -2.0, 0.5]), np.array([0.25, 0.0, -1.0]), np.array([5.0, 7.0, 11.0]))


def _engine(arrs):
    eng = bh_amd.Engine(bh_amd.default_params(), device=0)
    eng.reset_bodies(*arrs)
    return eng


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.int64)


def _assert_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}"


def _ms(eng, name):
    """(rc, value) of bh_<name>_kernel_ms through the raw ABI; the value starts as a canary."""
    ms = ctypes.c_double(-7.0)
    rc = getattr(eng._lib, f"bh_{name}_kernel_ms")(eng._h, ctypes.byref(ms))
    return rc, ms.value


# stopwatch -> a call of the query it times / a call of that query that launches nothing
_ONE = np.array([1000.0]), np.array([400.0])
_NONE = np.zeros(0), np.zeros(0)
TIMED = {
    "potential": lambda e: e.compute_potential(),
    "field": lambda e: e.compute_field(*_ONE),
    "direct_field": lambda e: e.compute_field_direct(*_ONE),
    "field_grid": lambda e: e.compute_field_grid(3.1, 3.3, 37.7, 24.3, 2, 2),
    "render": lambda e: e.render_bodies(width=64, height=32),
    "render_quads": lambda e: e.render_quads(width=64, height=32),
}
UNTIMED = {
    "field": [lambda e: e.compute_field(*_NONE)],
    "direct_field": [lambda e: e.compute_field_direct(*_NONE),
                     lambda e: e.force_error(idx=np.zeros(0, dtype=np.int64))],
    "render": [lambda e: e.render_tracers(width=64, height=32)],
}


@pytest.mark.parametrize("name", sorted(TIMED))
def test_stopwatch(name):
    eng = _engine(_three())
    if name == "render":
        eng.set_tracers(np.array([800.0, 1500.0]), np.array([250.0, 450.0]))
    fn = getattr(eng._lib, f"bh_{name}_kernel_ms")
    assert fn(eng._h, None) == bh_amd.BH_E_INVALID
    assert fn(None, ctypes.byref(ctypes.c_double(0.0))) == bh_amd.BH_E_INVALID
    assert _ms(eng, name) == (bh_amd.BH_OK, 0.0)  # nothing launched yet: exactly 0.0
    for quiet in UNTIMED.get(name, []):
        quiet(eng)
        assert _ms(eng, name) == (bh_amd.BH_OK, 0.0), "a call without a launch started the watch"
    TIMED[name](eng)
    rc, first = _ms(eng, name)
    assert rc == bh_amd.BH_OK and math.isfinite(first) and first >= 0.0, (rc, first)
    for quiet in UNTIMED.get(name, []):
        quiet(eng)
        assert _ms(eng, name) == (bh_amd.BH_OK, first), "a call without a launch moved the watch"
    assert fn(eng._h, None) == bh_amd.BH_E_INVALID
    eng.close()


def test_force_error_times_the_direct_kernel():
    eng = _engine(_three())
    assert _ms(eng, "direct_field") == (bh_amd.BH_OK, 0.0)
    eng.force_error(idx=np.array([2, 0], dtype=np.int64))
    rc, ms = _ms(eng, "direct_field")
    assert rc == bh_amd.BH_OK and math.isfinite(ms) and ms >= 0.0, (rc, ms)
    eng.close()


def _refusals():
    """(id, call(lib, handle, keep) -> rc, the exact bh_last_error text)."""
    one = np.array([1000.0])
    d = one.ctypes.data_as(_D)
    out = []
    for fn in ("bh_compute_field", "bh_compute_field_direct"):
        def call(lib, h, n, px, py, fn=fn):
            return getattr(lib, fn)(h, n, px, py, None, None, None, None)
        text = f"{fn}: n_probe must be in [0, 2^28]"
        out += [(f"{fn}-negative", lambda lib, h, c=call: c(lib, h, -1, d, d), text),
                (f"{fn}-too-many", lambda lib, h, c=call: c(lib, h, TOO_MANY, None, None), text),
                (f"{fn}-px-null", lambda lib, h, c=call: c(lib, h, 1, None, d),
                 f"{fn}: px or py is NULL"),
                (f"{fn}-py-null", lambda lib, h, c=call: c(lib, h, 1, d, None),
                 f"{fn}: px or py is NULL")]

    def tracers(lib, h, n, x, y):
        return lib.bh_set_tracers(h, n, x, y, None, None)
    text = "bh_set_tracers: n must be in [0, 2^28]"
    out += [("bh_set_tracers-negative", lambda lib, h: tracers(lib, h, -1, d, d), text),
            ("bh_set_tracers-too-many", lambda lib, h: tracers(lib, h, TOO_MANY, None, None), text),
            ("bh_set_tracers-x-null", lambda lib, h: tracers(lib, h, 1, None, d),
             "bh_set_tracers: x or y is NULL"),
            ("bh_set_tracers-y-null", lambda lib, h: tracers(lib, h, 1, d, None),
             "bh_set_tracers: x or y is NULL")]

    idx0 = np.array([0], dtype=np.int64)
    idx7 = np.array([0, 7, 1], dtype=np.int64)

    def ferr(lib, h, n, idx):
        s = bh_amd.BhForceError()
        p = idx.ctypes.data_as(_I64P) if idx is not None else None
        return lib.bh_compute_force_error(h, n, p, None, None, None, None, ctypes.byref(s))
    text = "bh_compute_force_error: n_sample must be in [0, 2^28]"
    out += [("bh_compute_force_error-negative", lambda lib, h: ferr(lib, h, -1, idx0), text),
            ("bh_compute_force_error-too-many", lambda lib, h: ferr(lib, h, TOO_MANY, None), text),
            ("bh_compute_force_error-idx-null", lambda lib, h: ferr(lib, h, 1, None),
             "bh_compute_force_error: idx is NULL"),
            ("bh_compute_force_error-idx-range", lambda lib, h: ferr(lib, h, 3, idx7),
             "bh_compute_force_error: idx[1] = 7 is outside [0, 3)")]
    return out


_REFUSALS = _refusals()


@pytest.mark.parametrize("call,text", [r[1:] for r in _REFUSALS], ids=[r[0] for r in _REFUSALS])
def test_refusal(call, text):
    eng = _engine(_three())
    before = eng.get_bodies()
    assert call(eng._lib, eng._h) == bh_amd.BH_E_INVALID
    assert eng._lib.bh_last_error(eng._h).decode() == text
    after = eng.get_bodies()
    for name, a, b in zip(FIELDS, after, before):
        _assert_bits(a, b, name)
    assert eng.num_tracers() == 0
    eng.close()


def _fresh_answer(bodies, query):
    """`query` on a new engine that holds `bodies`."""
    twin = _engine(bodies)
    try:
        return query(twin)
    finally:
        twin.close()


def _flatten(res):
    """A query's result as a list of (name, float64 array): None planes dropped, ctypes
    structures and dataclasses of scalars by field."""
    if isinstance(res, bh_amd.ForceError):
        planes = [("ax_tree", res.ax_tree), ("ay_tree", res.ay_tree), ("ax_exact", res.ax_exact),
                  ("ay_exact", res.ay_exact)]
        nums = [res.n_sample, res.n_used, res.worst, res.max_rel, res.mean_rel, res.rms_rel]
        return planes + [("summary", np.array(nums, dtype=np.float64))]
    out = []
    for k, a in enumerate(res):
        if a is None:
            continue
        if isinstance(a, ctypes.Structure):
            a = np.array([getattr(a, f) for f, _ in a._fields_], dtype=np.float64)
        out.append((f"[{k}]", a))
    return out


def test_kept_buffers_answer_as_fresh_ones():
    """1, 65, 1: the second call grows the planes past one wavefront, the third reads planes that
    keep the larger stride."""
    eng = _engine(scenes.uniform(200, 3.0, seed=11))
    rng = np.random.default_rng(5)
    px, py = rng.uniform(50.0, 2350.0, 66), rng.uniform(50.0, 750.0, 66)
    pm = rng.uniform(0.5, 2.0, 66)
    idx = rng.integers(0, 200, 66).astype(np.int64)
    cuts = [slice(0, 1), slice(1, 66), slice(7, 8)]  # 1, 65, 1 entries, never the same ones
    grids = [(1, 1), (9, 8), (1, 1)]
    sequences = {
        "field": [lambda e, c=c: e.compute_field(px[c], py[c], pm[c]) for c in cuts],
        "field_direct": [lambda e, c=c: e.compute_field_direct(px[c], py[c], pm[c]) for c in cuts],
        "force_error": [lambda e, c=c: e.force_error(idx=idx[c]) for c in cuts],
        "field_grid": [lambda e, g=g, k=k: e.compute_field_grid(
            3.1 + 100.0 * k, 3.3, 37.7, 24.3, g[0], g[1], want_stats=True)
            for k, g in enumerate(grids)],
    }
    for name, calls in sequences.items():
        for k, query in enumerate(calls):
            bodies = eng.get_bodies()
            got = _flatten(query(eng))
            want = _flatten(_fresh_answer(bodies, query))
            assert [g[0] for g in got] == [w[0] for w in want], f"{name} call {k}"
            for (plane, g), (_, w) in zip(got, want):
                _assert_bits(g, w, f"{name} call {k} {plane}")
    eng.close()
