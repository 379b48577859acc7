"""A breadth-first model of one body's walk -- TEST INFRASTRUCTURE ONLY.

The reference walks its tree depth first (BHA:215-239).  The engine's breadth-first walk
(traverse.hip bfs_walk) visits the same nodes level by level: every child of an opened cell is
either opened in turn, for the next level, or accepted -- a bit in a bitmap over node indices,
leaves included, the body's own leaf too.  It keeps at most BFS_E_CAP opened cells per level and
BFS_A_CAP accepted nodes, and falls back to the depth-first cursor walk beyond either, or when
the tree has more nodes than the bitmap has bits.  Which of those a body meets is a property of
the reference's tree alone, so this model reads it off oracle/py_oracle.py's BHTree:

  * a node with mass == 0.0 is skipped and not counted (BHA:216);
  * a leaf is accepted (BHA:217-223, the own leaf as well: the device marks it and drops the
    term later);
  * an internal node with s^2 < theta^2 * dist^2 is accepted, any other opened (BHA:224-237).

Opened plus accepted nodes of a body is therefore the reference's visit count, which pins the
model (tests/test_launch_plan.py).  The device additionally marks the empty children and the
jitter cells it keeps as skip slots; tests leave a factor of two for those.
"""
from __future__ import annotations

import sys

import numpy as np

from oracle import py_oracle


class FlatTree:
    """py_oracle.BHTree in arrays, nodes with mass != 0 only (pre-order)."""

    def __init__(self, root):
        mass, cx, cy, s2, leaf, kids = [], [], [], [], [], []
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 10_000))
        try:
            self._add(root, mass, cx, cy, s2, leaf, kids)
        finally:
            sys.setrecursionlimit(limit)
        self.mass = np.array(mass, dtype=np.float64)
        self.comX = np.array(cx, dtype=np.float64)
        self.comY = np.array(cy, dtype=np.float64)
        self.s2 = np.array(s2, dtype=np.float64)
        self.leaf = np.array(leaf, dtype=bool)
        self.kids = np.array(kids, dtype=np.int64).reshape(-1, 4)  # -1: none or massless

    def _add(self, node, mass, cx, cy, s2, leaf, kids):
        if node.mass == 0.0:
            return -1
        at = len(mass)
        mass.append(node.mass)
        cx.append(node.comX)
        cy.append(node.comY)
        s = node.quad.h * 2.0  # BHA:226
        s2.append(s * s)
        leaf.append(node.is_leaf())
        kids.append([-1, -1, -1, -1])
        if not node.is_leaf():
            kids[at] = [self._add(c, mass, cx, cy, s2, leaf, kids) for c in node.children]
        return at

    @property
    def nodes(self):
        return len(self.mass)


class WalkCounts:
    """opened[i][l]: cells body i opens on level l (root = level 0); accepted[i]: nodes it accepts;
    nodes: the tree's node count (mass != 0)."""

    def __init__(self, bodies, opened, accepted, nodes):
        self.bodies = bodies
        self.opened = opened
        self.accepted = accepted
        self.nodes = nodes

    @property
    def max_opened(self):  # per body: the widest level
        return self.opened.max(axis=1)

    @property
    def visits(self):  # per body: the reference's count (BHA:216 passed)
        return self.opened.sum(axis=1) + self.accepted


def build(arrs, theta=0.5, soft2=1.0, width_px=2400, height_px=800):
    """The reference's tree of the scene (with its jitter applied to the copies of the bodies):
    (FlatTree, x, y) -- positions as the walk sees them."""
    cfg = {"G": 80.0, "dt": 0.005, "theta": theta, "soft2": soft2, "width_px": width_px,
           "height_px": height_px}
    eng = py_oracle.make_engine(*arrs, cfg)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10_000))
    try:
        root = eng.build_tree()
    finally:
        sys.setrecursionlimit(limit)
    x = np.array([b.x for b in eng.bodies], dtype=np.float64)
    y = np.array([b.y for b in eng.bodies], dtype=np.float64)
    return FlatTree(root), x, y


def walk_counts(arrs, theta=0.5, soft2=1.0, bodies=None, width_px=2400, height_px=800,
                chunk=256):
    """Breadth-first walk of every body in `bodies` (default: all) over the reference's tree."""
    tree, x, y = build(arrs, theta, soft2, width_px, height_px)
    n = len(x)
    bodies = np.arange(n, dtype=np.int64) if bodies is None else np.asarray(bodies, np.int64)
    theta2 = theta * theta
    levels = []  # per level: opened cells of every walked body
    accepted = np.zeros(len(bodies), dtype=np.int64)
    if tree.nodes == 0:
        return WalkCounts(bodies, np.zeros((len(bodies), 1), np.int64), accepted, 0)
    for c0 in range(0, len(bodies), chunk):
        who = np.arange(c0, min(c0 + chunk, len(bodies)), dtype=np.int64)
        b = who.copy()                       # frontier: (walked body, node) pairs
        k = np.zeros(len(who), dtype=np.int64)
        level = 0
        while len(b):
            bx, by = x[bodies[b]], y[bodies[b]]
            dx = tree.comX[k] - bx
            dy = tree.comY[k] - by
            dist2 = dx * dx + dy * dy + soft2
            acc = tree.leaf[k] | (tree.s2[k] < theta2 * dist2)
            np.add.at(accepted, b[acc], 1)
            ob, ok = b[~acc], k[~acc]
            if level == len(levels):
                levels.append(np.zeros(len(bodies), dtype=np.int64))
            np.add.at(levels[level], ob, 1)
            kid = tree.kids[ok]              # (m, 4)
            b = np.repeat(ob, 4)
            k = kid.reshape(-1)
            live = k >= 0
            b, k = b[live], k[live]
            level += 1
    opened = np.stack(levels, axis=1)
    return WalkCounts(bodies, opened, accepted, tree.nodes)
