"""The checker of the field query (bh_compute_field) and its own cross-checks, on CPU.

`field_walk(root, px, py, pm, cfg)` is the reference's own walk for a body that is not in the
tree: the force is oracle.py_oracle.BHTree.accumulate_force called with a fresh py_oracle.Body
(its identity test never matches, so every non-empty leaf is taken), divided by pm; phi is
test_potential_ref._walk with that same fresh body, -(G * s).  No physics is restated here.
tests/test_gpu_field.py checks the engine bit for bit against it.
"""
import math
import os
import re

import numpy as np

import bh_amd
import oracle
from bh_amd import scenes
from oracle import py_oracle
from test_potential_ref import _walk, build, cfg_from_golden, checker_phi, make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = ("x", "y", "vx", "vy", "m")


def field_walk(root, px, py, pm, cfg):
    """(ax, ay, phi) of a probe Body(px, py, 0, 0, pm) that is not in the tree under `root`.
    The two divisions by pm are IEEE (0 / 0 = NaN), as the engine's are."""
    b = py_oracle.Body(float(px), float(py), 0.0, 0.0, float(pm))
    theta2 = cfg["theta"] * cfg["theta"]
    acc = [0.0, 0.0, 0]
    root.accumulate_force(b, theta2, acc, cfg)
    with np.errstate(all="ignore"):
        ax = float(np.float64(acc[0]) / np.float64(b.m))  # BHA:390-391
        ay = float(np.float64(acc[1]) / np.float64(b.m))
    s = [0.0]
    _walk(root, b, theta2, cfg["soft2"], s)
    return ax, ay, -(cfg["G"] * s[0])


def checker_field(arrs, cfg, px, py, pm=None):
    """(ax, ay, phi per probe, state after the build) by field_walk on the tree of `arrs`."""
    pe, root = build(arrs, cfg)
    out = np.empty((3, len(px)), dtype=np.float64)
    for j in range(len(px)):
        out[:, j] = field_walk(root, px[j], py[j], 1.0 if pm is None else pm[j], cfg)
    st = tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(pe))
    return out[0], out[1], out[2], st


def root_cell(cfg):
    """(cx, cy, h) of the root cell (BHA:360-361)."""
    w, h = cfg["width_px"], cfg["height_px"]
    return w / 2.0, h / 2.0, max(w, h) / 2.0 + 2.0


def make_probes(arrs, cfg, n, seed, on_bodies=True):
    """n probe points in a fixed mix, shuffled: uniform in the root cell, a clump within 3 units
    of the heaviest body (a disk centre), ~5 % outside the root cell, ~2 % exactly on body
    positions (of `arrs`: bodies the build does not jitter stay there; on_bodies=False: none)."""
    rng = np.random.default_rng(seed)
    cx, cy, h = root_cell(cfg)
    x, y, m = arrs[0], arrs[1], arrs[4]
    n_out = max(1, n // 20) if n >= 4 else 0
    n_on = max(1, n // 50) if on_bodies and n >= 4 and len(x) else 0
    n_clump = n // 4 if len(x) else 0
    n_uni = n - n_out - n_on - n_clump
    px = [rng.uniform(cx - h, cx + h, n_uni)]
    py = [rng.uniform(cy - h, cy + h, n_uni)]
    if n_clump:
        c = int(np.argmax(m))
        px.append(x[c] + rng.uniform(-3.0, 3.0, n_clump))
        py.append(y[c] + rng.uniform(-3.0, 3.0, n_clump))
    if n_out:
        side = rng.integers(0, 4, n_out)
        far = h * rng.uniform(1.0, 3.0, n_out) + 1.0
        along = rng.uniform(-h, h, n_out)
        px.append(np.where(side == 0, cx + far, np.where(side == 1, cx - far, cx + along)))
        py.append(np.where(side == 2, cy + far, np.where(side == 3, cy - far, cy + along)))
    if n_on:
        on = rng.choice(len(x), n_on, replace=False)
        px.append(x[on].copy())
        py.append(y[on].copy())
    px, py = np.concatenate(px), np.concatenate(py)
    order = rng.permutation(n)
    return np.ascontiguousarray(px[order]), np.ascontiguousarray(py[order])


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


# ---- the checker against the oracles --------------------------------------------------------

def test_outside_root_bodies_are_probes_of_their_own_mass():
    """A body outside the root cell is never inserted (BHA:126) but walked: the C oracle's
    acceleration for it, and the potential checker's phi, are the field at its position for a
    probe of its mass."""
    z = np.load(os.path.join(GOLDEN, "outside_153.npz"))
    arrs = tuple(z[f"init_{f}"] for f in FIELDS)
    cfg = cfg_from_golden(z)
    cx, cy, h = root_cell(cfg)
    outside = np.flatnonzero((np.abs(arrs[0] - cx) >= h) | (np.abs(arrs[1] - cy) >= h))
    assert outside.size > 0
    ref = oracle.Oracle(*arrs, p=oracle.params(**cfg))
    oax, oay = ref.accelerations()
    ref.close()
    phi, st = checker_phi(arrs, cfg)
    _, root = build(arrs, cfg)
    for i in outside:
        assert st[0][i] == arrs[0][i] and st[1][i] == arrs[1][i]  # (not inserted: not jittered)
        ax, ay, p = field_walk(root, arrs[0][i], arrs[1][i], arrs[4][i], cfg)
        assert _bits(ax) == _bits(oax[i]) and _bits(ay) == _bits(oay[i]), i
        assert _bits(p) == _bits(phi[i]), i


def test_coincident_probe_gets_the_self_term():
    """A probe exactly on an in-tree body differs from that body by the own leaf alone: phi gains
    the body's full term -G m / sqrt(soft2), the force gains a term of exactly zero."""
    arrs = scenes.two_disks(300, 100)
    cfg = make_cfg(theta=0.5, soft2=1.0)
    phi, st = checker_phi(arrs, cfg)
    _, root = build(arrs, cfg)
    for i in (0, 1, 57, 300, 399):
        ax, ay, p = field_walk(root, st[0][i], st[1][i], st[4][i], cfg)
        assert math.isfinite(ax) and math.isfinite(ay)
        assert p < phi[i]
        self_term = cfg["G"] * st[4][i] / math.sqrt(cfg["soft2"])
        # both sums have at most N + 1 terms of one sign: their roundings stay below this
        bound = (len(st[0]) + 17) * 2.0 ** -53 * abs(p)
        assert abs((phi[i] - p) - self_term) <= 2.0 * bound, (i, phi[i], p, self_term)


def test_two_bodies_known_answer():
    """A probe of mass 3 on body 0 of a pair: every cell that holds both bodies is opened (its
    side is at least the bodies' separation), so the sums are the two leaves'."""
    arrs = (np.array([100.0, 103.0]), np.array([100.0, 104.0]), np.zeros(2), np.zeros(2),
            np.array([1.0, 2.0]))
    cfg = make_cfg(theta=0.5, G=80.0, soft2=1.0, merge_min_dist=0.0)
    _, root = build(arrs, cfg)
    ax, ay, phi = field_walk(root, 100.0, 100.0, 3.0, cfg)
    r3 = 26.0 * math.sqrt(26.0)
    np.testing.assert_allclose([ax, ay, phi],
                               [80.0 * 2.0 * 3.0 / r3, 80.0 * 2.0 * 4.0 / r3,
                                -80.0 * (1.0 + 2.0 / math.sqrt(26.0))], rtol=1e-15, atol=0.0)
    # per unit mass, away from both bodies, theta = 0: the softened pair sums
    cfg0 = make_cfg(theta=0.0, G=80.0, soft2=1.0, merge_min_dist=0.0)
    ax, ay, phi = field_walk(root, 97.0, 96.0, 1.0, cfg0)
    want_ax = 80.0 * (1.0 * 3.0 / (26.0 * math.sqrt(26.0)) + 2.0 * 6.0 / (101.0 * math.sqrt(101.0)))
    want_ay = 80.0 * (1.0 * 4.0 / (26.0 * math.sqrt(26.0)) + 2.0 * 8.0 / (101.0 * math.sqrt(101.0)))
    want_phi = -80.0 * (1.0 / math.sqrt(26.0) + 2.0 / math.sqrt(101.0))
    np.testing.assert_allclose([ax, ay, phi], [want_ax, want_ay, want_phi], rtol=1e-15, atol=0.0)


def test_empty_tree_and_massless_probe():
    empty = tuple(np.zeros(0) for _ in range(5))
    cfg = make_cfg(theta=0.5)
    _, root = build(empty, cfg)
    ax, ay, phi = field_walk(root, 10.0, 20.0, 1.0, cfg)
    assert (ax, ay) == (0.0, 0.0) and math.copysign(1.0, ax) == 1.0
    assert phi == 0.0 and math.copysign(1.0, phi) == -1.0  # -(G * 0.0)
    arrs = scenes.two_disks(60, 20)
    _, root = build(arrs, cfg)
    ax, ay, phi = field_walk(root, 10.0, 20.0, 0.0, cfg)
    assert math.isnan(ax) and math.isnan(ay)
    assert _bits(phi) == _bits(field_walk(root, 10.0, 20.0, 1.0, cfg)[2])


def test_probe_mix_covers_every_kind():
    arrs = scenes.two_disks(1500, 500)
    cfg = make_cfg(theta=0.5)
    px, py = make_probes(arrs, cfg, 2000, 7)
    cx, cy, h = root_cell(cfg)
    outside = (np.abs(px - cx) >= h) | (np.abs(py - cy) >= h)
    assert 80 <= outside.sum() <= 120
    on = np.isin(px.view(np.int64), arrs[0].view(np.int64)) & \
        np.isin(py.view(np.int64), arrs[1].view(np.int64))
    assert 30 <= on.sum() <= 50
    c = int(np.argmax(arrs[4]))
    assert (np.hypot(px - arrs[0][c], py - arrs[1][c]) < 5.0).sum() >= 500


def test_header_declares_the_field_symbols():
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("bh_compute_field", "bh_field_kernel_ms"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert name in bh_amd.EXPORTED_SYMBOLS
    # the header documents what a probe is and whose tree and state semantics the call has
    assert "not in the tree" in txt and "bh_compute_potential's" in txt
