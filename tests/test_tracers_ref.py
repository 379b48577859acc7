"""The checkers of the tracers (bh_set_tracers: massless test particles stepped with the bodies)
and their own cross-checks, on CPU.

`tracer_steps(arrs, cfg, tx, ty, tvx, tvy, k)` is oracle.py_oracle.PhysicsEngine.step() restated
in its control flow only: after each compute_accelerations(root) it calls root.accumulate_force
for a py_oracle.Body(x, y, vx, vy, 1.0) per tracer -- a body that is in no tree, so its identity
test never matches and every non-empty leaf is taken -- and applies the step's own kick and drift
lines to it.  No physics is restated.

`tracer_steps_vec` is the same for many tracers at once in numpy: the tree flattened in pre-order
(massless nodes dropped, next[k] the index after k's subtree), one loop over the nodes with a
per-tracer skip index, one IEEE operation per numpy operation.  It exists because the recursive
checker is too slow at the sizes where the full-wave launch shapes begin.

tests/test_gpu_tracers.py checks the engine bit for bit against both.
"""
import os
import re

import numpy as np

import bh_amd
import oracle
from bh_amd import scenes
from oracle import py_oracle
from test_field_ref import make_probes, root_cell
from test_potential_ref import make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")


def _state(pe):
    return tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(pe))


def _f64(*arrs):
    return tuple(np.array(a, dtype=np.float64) for a in arrs)


def tracer_steps(arrs, cfg, tx, ty, tvx, tvy, k):
    """((tx, ty, tvx, tvy), body state) after k PhysicsEngine.step() calls with the tracers
    carried along.  soft2 must be > 0 wherever a tracer can sit on a centre of mass: Python
    raises on 1.0 / 0.0 where the engine's arithmetic gives inf."""
    pe = py_oracle.make_engine(*arrs, cfg)
    tr = [py_oracle.Body(float(tx[i]), float(ty[i]), float(tvx[i]), float(tvy[i]), 1.0)
          for i in range(len(tx))]
    theta2 = cfg["theta"] * cfg["theta"]
    dt = cfg["dt"]
    dt_half = dt * 0.5

    def walk(root):
        out = []
        for t in tr:
            acc = [0.0, 0.0, 0]
            root.accumulate_force(t, theta2, acc, cfg)
            out.append((acc[0] / t.m, acc[1] / t.m))  # BHA:390-391
        return out

    for _ in range(k):  # PhysicsEngine.step(), BHA:405-439
        root = pe.build_tree()
        ax, ay = pe.compute_accelerations(root)
        ta = walk(root)
        for i, b in enumerate(pe.bodies):
            b.vx += ax[i] * dt_half
            b.vy += ay[i] * dt_half
        for b in pe.bodies:
            b.x += b.vx * dt
            b.y += b.vy * dt
        for t, (a, c) in zip(tr, ta):
            t.vx += a * dt_half
            t.vy += c * dt_half
            t.x += t.vx * dt
            t.y += t.vy * dt
        root = pe.build_tree()
        ax, ay = pe.compute_accelerations(root)
        ta = walk(root)
        for i, b in enumerate(pe.bodies):
            b.vx += ax[i] * dt_half
            b.vy += ay[i] * dt_half
        for t, (a, c) in zip(tr, ta):
            t.vx += a * dt_half
            t.vy += c * dt_half
        pe.last_tree = root
        pe.merge_close_bodies_if_needed()
    return _f64([t.x for t in tr], [t.y for t in tr], [t.vx for t in tr],
                [t.vy for t in tr]), _state(pe)


def flatten(root):
    """The tree in pre-order without its massless nodes (BHA:216 returns there): per node
    (comX, comY, mass, is_leaf, s2, next), next = the index after the node's subtree."""
    recs = []

    def rec(node):
        if node.mass == 0.0:
            return
        k = len(recs)
        recs.append(None)
        if not node.is_leaf():
            for c in node.children:
                rec(c)
        s = node.quad.h * 2.0  # BHA:226
        recs[k] = (node.comX, node.comY, node.mass, node.is_leaf(), s * s, len(recs))

    rec(root)
    return recs


def walk_vec(flat, tx, ty, cfg):
    """(ax, ay) of every tracer over the flattened tree: accumulate_force for a body of mass 1.0
    that is in no leaf, the terms of _point_force_acc in its order."""
    theta2 = cfg["theta"] * cfg["theta"]
    soft2, Gm = cfg["soft2"], cfg["G"] * 1.0
    fx = np.zeros(len(tx), dtype=np.float64)
    fy = np.zeros(len(tx), dtype=np.float64)
    skip = np.zeros(len(tx), dtype=np.int64)  # the tracer is active at node k iff skip <= k
    with np.errstate(all="ignore"):
        for k, (cx, cy, m, leaf, s2, nxt) in enumerate(flat):
            act = np.flatnonzero(skip <= k)  # (only these are computed: the others skip k)
            if act.size == 0:
                continue
            dx = cx - tx[act]
            dy = cy - ty[act]
            r2 = dx * dx + dy * dy + soft2
            if not leaf:  # BHA:226-228; a NaN compares false: the node is opened
                take = s2 < theta2 * r2
                act, dx, dy, r2 = act[take], dx[take], dy[take], r2[take]
            inv_r = 1.0 / np.sqrt(r2)
            inv_r2 = 1.0 / r2
            f = Gm * m * inv_r2
            fx[act] = fx[act] + f * dx * inv_r
            fy[act] = fy[act] + f * dy * inv_r
            skip[act] = nxt
        return fx / 1.0, fy / 1.0


def tracer_steps_vec(arrs, cfg, tx, ty, tvx, tvy, k):
    """tracer_steps with the tracers in numpy arrays."""
    pe = py_oracle.make_engine(*arrs, cfg)
    tx, ty, tvx, tvy = _f64(tx, ty, tvx, tvy)
    dt = cfg["dt"]
    dt_half = dt * 0.5
    with np.errstate(all="ignore"):
        for _ in range(k):  # PhysicsEngine.step(), BHA:405-439
            root = pe.build_tree()
            ax, ay = pe.compute_accelerations(root)
            tax, tay = walk_vec(flatten(root), tx, ty, cfg)
            for i, b in enumerate(pe.bodies):
                b.vx += ax[i] * dt_half
                b.vy += ay[i] * dt_half
            for b in pe.bodies:
                b.x += b.vx * dt
                b.y += b.vy * dt
            tvx = tvx + tax * dt_half
            tvy = tvy + tay * dt_half
            tx = tx + tvx * dt
            ty = ty + tvy * dt
            root = pe.build_tree()
            ax, ay = pe.compute_accelerations(root)
            tax, tay = walk_vec(flatten(root), tx, ty, cfg)
            for i, b in enumerate(pe.bodies):
                b.vx += ax[i] * dt_half
                b.vy += ay[i] * dt_half
            tvx = tvx + tax * dt_half
            tvy = tvy + tay * dt_half
            pe.last_tree = root
            pe.merge_close_bodies_if_needed()
    return (tx, ty, tvx, tvy), _state(pe)


def outside_tracers(cfg, n, seed, speed=5.0):
    """n tracers at least 1 unit outside the root cell -- on all four sides, up to one root
    half-width away -- with speeds of at most `speed` in each component."""
    rng = np.random.default_rng(seed)
    cx, cy, h = root_cell(cfg)
    side = rng.integers(0, 4, n)
    far = h + 1.0 + h * rng.random(n)
    along = rng.uniform(-h, h, n)
    tx = np.where(side == 0, cx + far, np.where(side == 1, cx - far, cx + along))
    ty = np.where(side == 2, cy + far, np.where(side == 3, cy - far, cy + along))
    tvx = rng.uniform(-speed, speed, n)
    tvy = rng.uniform(-speed, speed, n)
    return tx, ty, tvx, tvy


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def assert_same(got, want, what):
    for name, g, w in zip(("x", "y", "vx", "vy", "m"), got, want):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape, f"{what} {name}: shape {g.shape} vs {w.shape}"
        bad = np.flatnonzero(_bits(g) != _bits(w))
        assert bad.size == 0, (f"{what} {name}: {bad.size} words differ, first at {bad[:5]}: "
                               f"{g[bad[:3]]} vs {w[bad[:3]]}")


def oracle_with_appended(arrs, cfg, tr, k):
    """(tracers, bodies) of the C oracle after k steps on the body list with the tracers
    appended as bodies of mass 1.0.  Outside the root cell, and farther than mergeMinDist from
    every heavy body, the reference neither inserts nor merges them: they are tracers."""
    n = len(arrs[0])
    full = tuple(np.concatenate([a, t]) for a, t in
                 zip(arrs, (*tr, np.ones(len(tr[0])))))
    ref = oracle.Oracle(*full, p=oracle.params(**cfg))
    ref.step(k)
    out = ref.get_bodies()
    ref.close()
    nb = len(out[0]) - len(tr[0])  # (merges among the bodies shrink the front of the list)
    assert nb <= n
    return tuple(a[nb:] for a in out[:4]), tuple(a[:nb] for a in out)


# ---- the checkers against the oracle and each other --------------------------------------------

def test_tracer_steps_equals_the_oracle_on_appended_outside_bodies():
    for n1, n2 in ((600, 200), (300, 100)):
        arrs = scenes.two_disks(n1, n2)
        cfg = make_cfg(theta=0.5)
        tr = outside_tracers(cfg, 256, 5)
        heavy = np.flatnonzero(arrs[4] > cfg["merge_max_mass"])
        d = np.hypot(tr[0][:, None] - arrs[0][None, heavy], tr[1][:, None] - arrs[1][None, heavy])
        assert d.min() > cfg["merge_min_dist"] + 5.0 * 3 * cfg["dt"] + 1.0
        got_t, got_b = tracer_steps(arrs, cfg, *tr, 3)
        want_t, want_b = oracle_with_appended(arrs, cfg, tr, 3)
        assert_same(got_t, want_t, "tracers")
        assert_same(got_b, want_b, "bodies beside tracers")
        alone = oracle.Oracle(*arrs, p=oracle.params(**cfg))
        alone.step(3)
        assert_same(got_b, alone.get_bodies(), "bodies alone")
        alone.close()
        assert not any(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got_t, tr))


def edge_tracers(arrs, cfg, n, seed):
    """n tracers: the probe mix (inside the root cell, clumped at a disk centre, outside it, on
    bodies) with velocities, the last two at 2^40 and at 1e300."""
    tx, ty = make_probes(arrs, cfg, n, seed)
    rng = np.random.default_rng(seed + 1)
    tvx = rng.uniform(-30.0, 30.0, n)
    tvy = rng.uniform(-30.0, 30.0, n)
    tx[-2], ty[-2] = 2.0 ** 40, -(2.0 ** 40)
    tx[-1], ty[-1] = 1e300, 1e300
    return tx, ty, tvx, tvy


def test_tracer_steps_vec_equals_tracer_steps():
    arrs = scenes.two_disks(300, 100)
    cfg = make_cfg(theta=0.5)
    tr = edge_tracers(arrs, cfg, 500, 3)
    cx, cy, h = root_cell(cfg)
    outside = (np.abs(tr[0] - cx) >= h) | (np.abs(tr[1] - cy) >= h)
    on = np.isin(_bits(tr[0]), _bits(arrs[0])) & np.isin(_bits(tr[1]), _bits(arrs[1]))
    assert outside.sum() >= 20 and on.sum() >= 5 and (~outside).sum() >= 400
    a_t, a_b = tracer_steps(arrs, cfg, *tr, 2)
    b_t, b_b = tracer_steps_vec(arrs, cfg, *tr, 2)
    assert_same(b_t, a_t, "tracers")
    assert_same(b_b, a_b, "bodies")
    assert all(np.all(np.isfinite(a)) for a in a_t)


def test_flatten_drops_massless_nodes_and_links_subtrees():
    arrs = scenes.two_disks(60, 20)
    cfg = make_cfg(theta=0.5)
    pe = py_oracle.make_engine(*arrs, cfg)
    flat = flatten(pe.build_tree())
    assert all(r[2] != 0.0 for r in flat)
    assert flat[0][5] == len(flat)
    assert sum(1 for r in flat if r[3]) == len(arrs[0])  # every body is inside the root cell
    for k, r in enumerate(flat):
        assert k < r[5] <= len(flat) and (not r[3] or r[5] == k + 1)


def test_empty_tree_drifts_on_straight_lines():
    empty = tuple(np.zeros(0) for _ in range(5))
    cfg = make_cfg(theta=0.5)
    tr = (np.array([10.0, -3.0]), np.array([20.0, 5.0]), np.array([-0.0, 2.0]),
          np.array([1.0, -0.0]))
    for fn in (tracer_steps, tracer_steps_vec):
        (x, y, vx, vy), st = fn(empty, cfg, *tr, 2)
        assert len(st[0]) == 0
        # -0.0 + 0.0 * dtHalf = +0.0: the arithmetic's own answer
        assert_same((vx, vy), (np.array([0.0, 2.0]), np.array([1.0, 0.0])), fn.__name__)
        assert x[1] == -3.0 + 2.0 * cfg["dt"] + 2.0 * cfg["dt"] and x[0] == 10.0


# ---- the header and the binding ------------------------------------------------------------------

TRACER_SYMBOLS = ("bh_set_tracers", "bh_num_tracers", "bh_get_tracers", "bh_tracer_kernel_ms",
                  "bh_tracer_launch_shape", "bh_render_tracers")


def test_header_declares_the_tracer_symbols():
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in TRACER_SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, code), f"{name} not declared"
        assert name in bh_amd.EXPORTED_SYMBOLS
    # the contract: what a tracer is, the merge rule, the deliberate one-GPU limit, the calls
    # refused while a bh_step_begin call runs
    assert "never\n * inserted into any tree" in txt or "never inserted into any tree" in txt
    assert "Tracers never take part in the merge rule" in txt
    assert "locally essential trees, which a tracer cannot walk" in txt
    begin = txt[txt.index("bh_step(e, k) on a thread of the engine's own"):
                txt.index("int bh_step_begin")]
    for name in ("bh_set_tracers", "bh_get_tracers", "bh_render_tracers"):
        assert name in begin, f"{name} missing from the calls refused until bh_step_end"


def test_binding_has_the_tracer_methods():
    for name in ("set_tracers", "get_tracers", "num_tracers", "tracer_kernel_ms",
                 "render_tracers"):
        assert callable(getattr(bh_amd.Engine, name))
    assert callable(bh_amd.tracer_launch_shape)


def test_library_exports_and_launch_shape():
    lib = bh_amd.load_library()
    for name in TRACER_SYMBOLS:
        assert hasattr(lib, name), name
    # host-only: field_walk's shape, short one-wave groups for a handful, full waves for many
    few = bh_amd.tracer_launch_shape(1)
    assert 1 <= few[0] < 64 and few[1] == 1
    bpw, wpb, R = bh_amd.tracer_launch_shape(1 << 20)
    assert bpw == 64 and 1 <= wpb <= 8 and R >= 1
    assert bh_amd.tracer_launch_shape(5)[2] == R  # one compile-time constant
    for bad in (-1, (1 << 28) + 1):
        try:
            bh_amd.tracer_launch_shape(bad)
        except bh_amd.BhError as e:
            assert e.rc == bh_amd.BH_E_INVALID
        else:
            raise AssertionError(f"n = {bad} was accepted")
