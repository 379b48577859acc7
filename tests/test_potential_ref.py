"""The checker of the potential walk (bh_compute_potential) and its own cross-checks, on CPU.

`potential_walk(tree_root, body, cfg)` is a Python walk over oracle.py_oracle's BHTree that
visits exactly the nodes accumulate_force visits (BHA:215-239) and adds, per taken node in
pre-order,

    dx = comX - b.x; dy = comY - b.y; r2 = dx*dx + dy*dy + soft2
    s += mass * (1.0 / sqrt(r2))                                   (s from +0.0)

phi_b = -(G * s).  An accepted cell that contains b includes b's own mass, as its force does.
`theta0_phi` is the vectorised theta = 0 form: the leaves in pre-order, summed sequentially with
np.cumsum along the leaf axis (np.sum would add pairwise).  tests/test_gpu_potential.py checks
the engine bit for bit against these.
"""
import math
import os
import re

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from conftest import bits_equal
from oracle import py_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")


def make_cfg(**over):
    cfg = dict(G=80.0, dt=0.005, theta=0.30, soft2=1.0, width_px=2400, height_px=800,
               merge_max_mass=4000.0, merge_min_dist=8.0)
    cfg.update(over)
    return cfg


def cfg_from_golden(z):
    p = z["params"]
    return make_cfg(G=float(p[0]), dt=float(p[1]), theta=float(p[2]), soft2=float(p[3]),
                    width_px=int(p[4]), height_px=int(p[5]), merge_max_mass=float(p[6]),
                    merge_min_dist=float(p[7]))


def params_of(cfg):
    return bh_amd.default_params(**cfg)


def _walk(node, b, theta2, soft2, acc):
    if node.mass == 0.0:  # BHA:216
        return
    if node.is_leaf():
        if node.body is None or node.body is b:  # BHA:219: the own leaf, by identity
            return
        take = True
    else:
        dx = node.comX - b.x
        dy = node.comY - b.y
        dist2 = dx * dx + dy * dy + soft2
        s = node.quad.h * 2.0
        take = s * s < theta2 * dist2  # BHA:226-228, strict
    if take:
        dx = node.comX - b.x
        dy = node.comY - b.y
        r2 = dx * dx + dy * dy + soft2
        inv_r = 1.0 / math.sqrt(r2)
        acc[0] += node.mass * inv_r
        return
    for c in node.children:
        _walk(c, b, theta2, soft2, acc)


def potential_walk(tree_root, body, cfg):
    """phi of `body` over the tree (a body outside the root cell walks too)."""
    acc = [0.0]
    _walk(tree_root, body, cfg["theta"] * cfg["theta"], cfg["soft2"], acc)
    return -(cfg["G"] * acc[0])


def build(arrs, cfg):
    """(engine, root) after one buildTree() on `arrs` -- the jitter has moved the bodies."""
    pe = py_oracle.make_engine(*arrs, cfg)
    root = pe.build_tree()
    return pe, root


def checker_phi(arrs, cfg):
    """(phi per body, state after the build) by the Python walk."""
    pe, root = build(arrs, cfg)
    phi = np.array([potential_walk(root, b, cfg) for b in pe.bodies], dtype=np.float64)
    return phi, tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(pe))


def leaves_preorder(root):
    """The leaves a theta = 0 walk visits, in its order: bodies of non-massless leaves that
    lie under no massless node (BHA:216 returns there)."""
    out = []

    def rec(node):
        if node.mass == 0.0:
            return
        if node.is_leaf():
            if node.body is not None:
                out.append(node)
            return
        for c in node.children:
            rec(c)

    rec(root)
    return out


def theta0_phi(arrs, cfg):
    """(phi per body, state after the build): the theta = 0 sum over the leaf sequence,
    vectorised over (body, leaf) and added left to right along the leaf axis."""
    pe, root = build(arrs, cfg)
    leaves = leaves_preorder(root)
    lx = np.array([l.comX for l in leaves], dtype=np.float64)
    ly = np.array([l.comY for l in leaves], dtype=np.float64)
    lm = np.array([l.mass for l in leaves], dtype=np.float64)
    index = {id(b): i for i, b in enumerate(pe.bodies)}
    own = np.array([index[id(l.body)] for l in leaves], dtype=np.int64)
    st = tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(pe))
    bx, by = st[0], st[1]
    dx = lx[None, :] - bx[:, None]
    dy = ly[None, :] - by[:, None]
    r2 = dx * dx + dy * dy + cfg["soft2"]
    term = lm[None, :] * (1.0 / np.sqrt(r2))
    term[own, np.arange(len(leaves))] = 0.0  # the own leaf is skipped: s + 0.0 == s
    if len(leaves):
        s = np.cumsum(term, axis=1)[:, -1]
    else:
        s = np.zeros(len(bx))
    return -(cfg["G"] * s), st


def energy(state, phi):
    """(kinetic, potential) of a state and its phi, exactly rounded sums of the fp64 terms."""
    x, y, vx, vy, m = state
    ke = math.fsum((0.5 * m * (vx * vx + vy * vy)).tolist())
    pe = 0.5 * math.fsum((m * phi).tolist())
    return ke, pe


def sum_bound(terms):
    """Error bound of any-order fp64 summation of `terms` plus the terms' own roundings."""
    n = len(terms)
    return (n + 16) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())


# ---- the checker against itself ------------------------------------------------------------

def test_theta0_walk_equals_the_vectorised_form():
    arrs = scenes.two_disks(300, 100)
    cfg = make_cfg(theta=0.0)
    walk, st_w = checker_phi(arrs, cfg)
    vec, st_v = theta0_phi(arrs, cfg)
    assert bits_equal(walk, vec)
    for a, b in zip(st_w, st_v):
        assert bits_equal(a, b)


@pytest.mark.parametrize("case", ["soft2_0", "far"])
def test_theta0_walk_equals_the_vectorised_form_at_the_edges(case):
    """The two checkers against each other where the engine leaves its fast path: soft2 = 0
    (the own leaf's 1 / sqrt(0) must be skipped, not multiplied away) and bodies far outside
    the root cell (dx * dx overflows: 1 / sqrt(inf) = 0).  Every phi is finite."""
    from test_oracle import with_far_bodies
    arrs = scenes.two_disks(300, 100)
    cfg = make_cfg(theta=0.0)
    if case == "soft2_0":
        cfg["soft2"] = 0.0
    else:
        arrs = with_far_bodies(arrs)
    with np.errstate(over="ignore", divide="ignore"):
        walk, st_w = checker_phi(arrs, cfg)
        vec, st_v = theta0_phi(arrs, cfg)
    assert np.all(np.isfinite(walk))
    assert bits_equal(walk, vec)
    for a, b in zip(st_w, st_v):
        assert bits_equal(a, b)


def test_theta0_is_the_softened_pair_potential():
    arrs = scenes.two_disks(300, 100)
    cfg = make_cfg(theta=0.0)
    phi, st = checker_phi(arrs, cfg)
    x, y, _, _, m = (a.tolist() for a in st)
    n = len(x)
    for i in range(n):
        terms = [m[j] / math.sqrt((x[j] - x[i]) ** 2 + (y[j] - y[i]) ** 2 + cfg["soft2"])
                 for j in range(n) if j != i]
        want = -cfg["G"] * math.fsum(terms)
        bound = cfg["G"] * (n + 16) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
        assert abs(phi[i] - want) <= bound, (i, phi[i], want, bound)


def test_accepted_cells_include_the_own_mass():
    """Two bodies in one far-away cell, one observer: at a large theta the observer takes the
    pair's cell as one node, and each of the pair -- inside that cell -- opens it."""
    arrs = (np.array([100.0, 101.0, 2000.0]), np.array([100.0, 100.5, 700.0]), np.zeros(3),
            np.zeros(3), np.array([1.0, 2.0, 4.0]))
    cfg = make_cfg(theta=1.0)
    phi, st = checker_phi(arrs, cfg)
    pe, root = build(arrs, cfg)
    far = potential_walk(root, pe.bodies[2], cfg)
    assert far == phi[2]
    # the observer saw one node of mass 3 at the pair's centre of mass
    cx = (100.0 * 1.0 + 101.0 * 2.0) / 3.0
    cy = (100.0 * 1.0 + 100.5 * 2.0) / 3.0
    r2 = (cx - 2000.0) ** 2 + (cy - 700.0) ** 2 + 1.0
    assert math.isclose(far, -80.0 * 3.0 / math.sqrt(r2), rel_tol=1e-14)


def test_header_declares_the_new_symbols():
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("bh_compute_potential", "bh_compute_diagnostics", "bh_potential_kernel_ms",
                 "bh_nbody3d_center_of_mass"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert name in bh_amd.EXPORTED_SYMBOLS
    assert re.search(r"typedef\s+struct\s+bh_diagnostics\s*\{", code)
    body = re.search(r"typedef\s+struct\s+bh_diagnostics\s*\{(.*?)\}", code, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z]+)\s*[,;]", body)
    assert fields == [f for f, _ in bh_amd.BhDiagnostics._fields_]
    # the header documents the self-mass convention and the state semantics
    assert "own mass" in txt and "bh_compute_accelerations'" in txt


def test_diagnostics_dataclass_derives_com_energy_momentum():
    d = bh_amd.Diagnostics(n=2, mass=4.0, mx=8.0, my=-2.0, px=1.0, py=2.0, lz=0.5, kinetic=3.0,
                           potential=-5.0)
    assert d.com == (2.0, -0.5) and d.momentum == (1.0, 2.0) and d.energy == -2.0
    z = bh_amd.Diagnostics(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert z.com == (0.0, 0.0) and z.energy == 0.0
