"""The checker of the step log (bh_set_step_log) and its own cross-checks, on CPU.

`LogEngine` is oracle.py_oracle's PhysicsEngine with one hook: merge_close_bodies_if_needed --
which step() calls right after the second kick (BHA:432) with last_tree = the second
evaluation's root -- first records the step and then runs the parent's merge rule.  One record
holds, for the body list L at that point, the state planes, phi_b = potential_walk(root, b) of
every body (tests/test_potential_ref.py: accumulateForce's nodes, own leaf skipped, strict
criterion, terms in pre-order) and the exactly rounded sums (math.fsum) that a record's
bh_diagnostics approximates.  tests/test_gpu_step_log.py checks the engine against these.
"""
import ctypes
import math
import os
import re

import numpy as np

import bh_amd
from bh_amd import scenes
from conftest import bits_equal
from oracle import py_oracle
from test_potential_ref import (cfg_from_golden, checker_phi, energy, make_cfg, potential_walk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bh_engine.h")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("x", "y", "vx", "vy", "m")
SUMS = ("mass", "mx", "my", "px", "py", "lz", "kinetic", "potential")


def ieee_div(a, b):
    """a / b in IEEE binary64 (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return float("nan")
    return math.copysign(float("inf"), a) * math.copysign(1.0, b)


class LogEngine(py_oracle.PhysicsEngine):
    """PhysicsEngine that logs every step at BHA:432, before the merge rule (BHA:438)."""

    def __init__(self, bodies, cfg):
        super().__init__(bodies, cfg)
        self.log = []
        self.t = 0.0

    def compute_accelerations(self, root):
        """The parent's (BHA:374-395) with the JVM's division: F / m for m = 0.0 is NaN or an
        infinity (BHA:390-391), where Python raises."""
        theta2 = self.cfg["theta"] * self.cfg["theta"]
        ax, ay, vis = [], [], []
        for b in self.bodies:
            acc = [0.0, 0.0, 0]
            root.accumulate_force(b, theta2, acc, self.cfg)
            ax.append(ieee_div(acc[0], b.m))
            ay.append(ieee_div(acc[1], b.m))
            vis.append(acc[2])
        self.visits = vis
        return ax, ay

    def merge_close_bodies_if_needed(self):
        self.t += self.cfg["dt"]
        state = tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(self))
        root = self.last_tree
        phi = np.array([potential_walk(root, b, self.cfg) for b in self.bodies],
                       dtype=np.float64)
        self.log.append(dict(step=len(self.log) + 1, t=self.t, n=len(self.bodies), state=state,
                             phi=phi))
        super().merge_close_bodies_if_needed()


def reference_log(arrs, cfg, k):
    """(the records of k steps from `arrs`, the engine afterwards)."""
    pe = LogEngine([py_oracle.Body(*(float(a[i]) for a in arrs)) for i in range(len(arrs[0]))],
                   cfg)
    for _ in range(k):
        pe.step()
    return pe.log, pe


def record_terms(rec):
    """The fp64 terms of a record's sums, by bh_diagnostics field (`potential`: m * phi, whose
    sum the field halves)."""
    x, y, vx, vy, m = rec["state"]
    return {"mass": m, "mx": m * x, "my": m * y, "px": m * vx, "py": m * vy,
            "lz": m * (x * vy - y * vx), "kinetic": 0.5 * m * (vx * vx + vy * vy),
            "potential": m * rec["phi"]}


def build_moves_nothing(state, cfg):
    """Whether buildTree() on `state` leaves every position as it is (no jitter, BHA:146-151)."""
    pe = py_oracle.make_engine(*state, cfg)
    pe.build_tree()
    after = py_oracle.state(pe)
    return (bits_equal(np.array(after[0]), np.asarray(state[0], dtype=np.float64)) and
            bits_equal(np.array(after[1]), np.asarray(state[1], dtype=np.float64)))


def golden_start(name):
    z = np.load(os.path.join(GOLDEN, name))
    return tuple(z[f"init_{f}"] for f in FIELDS), cfg_from_golden(z)


# ---- the checker against itself ------------------------------------------------------------

def test_record_equals_the_potential_checker_on_a_quiet_scene():
    """No jitter, no merging: a re-build of the state after s steps is the step's second tree, so
    record s is checker_phi / energy of the oracle's state after s steps."""
    arrs = scenes.two_disks(100, 40)
    cfg = make_cfg(theta=0.5, merge_min_dist=0.0)
    log, _ = reference_log(arrs, cfg, 3)
    plain = py_oracle.make_engine(*arrs, cfg)
    t = 0.0
    for s in range(3):
        plain.step()
        t += cfg["dt"]
        now = tuple(np.array(a, dtype=np.float64) for a in py_oracle.state(plain))
        assert build_moves_nothing(now, cfg)
        phi, st = checker_phi(now, cfg)
        rec = log[s]
        assert (rec["step"], rec["t"], rec["n"]) == (s + 1, t, 140)
        assert bits_equal(rec["phi"], phi)
        for a, b in zip(rec["state"], st):
            assert bits_equal(a, b)
        ke, pe = energy(st, phi)
        terms = record_terms(rec)
        assert math.fsum(terms["kinetic"].tolist()) == ke
        assert 0.5 * math.fsum(terms["potential"].tolist()) == pe


def test_ieee_division():
    inf = float("inf")
    assert ieee_div(3.0, 2.0) == 1.5 and ieee_div(1.0, 0.0) == inf and ieee_div(-1.0, 0.0) == -inf
    assert ieee_div(1.0, -0.0) == -inf and math.isnan(ieee_div(0.0, 0.0))
    assert math.isnan(ieee_div(float("nan"), 0.0))


def test_records_precede_the_merge_rule():
    """merge_127: the list of a record is the one before its step's removals."""
    arrs, cfg = golden_start("merge_127.npz")
    log, pe = reference_log(arrs, cfg, 6)
    ns = [r["n"] for r in log]
    assert ns[0] == len(arrs[0]) and ns == sorted(ns, reverse=True)
    assert len(pe.bodies) <= ns[-1] and len(pe.bodies) < ns[0]
    # the hook changes nothing: the same bodies as the plain engine's
    plain = py_oracle.make_engine(*arrs, cfg)
    for _ in range(6):
        plain.step()
    for a, b in zip(py_oracle.state(pe), py_oracle.state(plain)):
        assert bits_equal(np.array(a), np.array(b))


# ---- the interface ---------------------------------------------------------------------------

NEW = ("bh_set_step_log", "bh_get_step_log", "bh_get_step_log_phi", "bh_step_log_kernel_ms")


def test_header_declares_the_step_log():
    txt = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
    body = re.search(r"typedef\s+struct\s+bh_step_record\s*\{(.*?)\}\s*bh_step_record\s*;", code,
                     flags=re.S)
    assert body, "struct bh_step_record not declared"
    assert re.findall(r"\b([a-z]+)\s*;", body.group(1)) == ["step", "t", "d"]
    assert re.search(r"int64_t\s+step\s*;\s*double\s+t\s*;\s*bh_diagnostics\s+d\s*;",
                     body.group(1))


def test_binding_exposes_the_step_log():
    for name in NEW:
        assert name in bh_amd.EXPORTED_SYMBOLS
    assert [f for f, _ in bh_amd.BhStepRecord._fields_] == ["step", "t", "d"]
    assert ctypes.sizeof(bh_amd.BhStepRecord) == 16 + ctypes.sizeof(bh_amd.BhDiagnostics) == 88
    for method in ("set_step_log", "get_step_log", "get_step_log_phi", "step_log_kernel_ms"):
        assert callable(getattr(bh_amd.Engine, method))
    d = bh_amd.Diagnostics(1, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0, -1.0)
    r = bh_amd.StepRecord(step=4, t=0.02, d=d)
    assert (r.step, r.t, r.d.energy) == (4, 0.02, 2.0)
