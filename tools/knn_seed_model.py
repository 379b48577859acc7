#!/usr/bin/env python3
"""How loose is bh_find_knn_bodies' seed?  A numpy model on the C3 start positions.

Usage (no GPU): python tools/knn_seed_model.py
Needs scipy (cKDTree gives the true k-th distance).  The bodies inside the root cell are put in
Morton order of the depth-21 grid, as the build's leaf sequence is, and for k = 8 and k = 32 the
seed radius of every body is formed as k_knn_seed forms it, in three variants:
  * centre      the largest distance in the one window of k + 1 leaves around the body,
  * three       the smallest of that and of the windows before and from the body on (the kernel),
  * union-kth   the k-th smallest distance over the 2 (k + 1) leaves on either side,
and `three` repaired inside each wave by the triangle inequality (seed_B + |AB|).
Printed per variant: the ratio seed radius / true d_k per lane (median, 99th percentile, largest)
and per wave of 64 consecutive lanes the largest ratio (median, 90th, 99th percentile) and the
mean of its square -- a wave walks as far as its worst lane, and the leaves it visits go with the
area.  A model: distances in plain binary64, no jitter, the start state only.
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "barnes-hut-n-body_amd"))
import bh_amd  # noqa: E402
from bh_amd import scenes  # noqa: E402

J = 21


def spread(v):
    v = v.astype(np.uint64)
    v = (v | (v << np.uint64(16))) & np.uint64(0x0000FFFF0000FFFF)
    v = (v | (v << np.uint64(8))) & np.uint64(0x00FF00FF00FF00FF)
    v = (v | (v << np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    v = (v | (v << np.uint64(2))) & np.uint64(0x3333333333333333)
    return (v | (v << np.uint64(1))) & np.uint64(0x5555555555555555)


def report(k, name, ratio):
    wave = ratio[:len(ratio) // 64 * 64].reshape(-1, 64).max(axis=1)
    print(f"k={k:2d} {name:15s} lane: median {np.median(ratio):5.2f} p99 "
          f"{np.percentile(ratio, 99):6.2f} max {ratio.max():7.1f} | wave's worst: median "
          f"{np.median(wave):5.2f} p90 {np.percentile(wave, 90):5.2f} p99 "
          f"{np.percentile(wave, 99):5.1f} mean square {np.mean(wave ** 2):7.1f}")


def main():
    p = bh_amd.default_params(theta=0.5)
    x, y, _, _, _ = scenes.config_scene("c3")
    cx, cy = p.width_px / 2.0, p.height_px / 2.0
    h = max(p.width_px, p.height_px) / 2.0 + 2.0
    w = 2.0 * h / 2 ** J
    ix, iy = np.floor((x - (cx - h)) / w), np.floor((y - (cy - h)) / w)
    inside = (ix >= 0) & (ix < 2 ** J) & (iy >= 0) & (iy < 2 ** J)
    x, y, ix, iy = x[inside], y[inside], ix[inside], iy[inside]
    order = np.argsort(spread(ix) | (spread(iy) << np.uint64(1)), kind="stable")
    x, y = x[order], y[order]
    n = len(x)
    me = np.arange(n)
    tree = cKDTree(np.c_[x, y])

    def dist(j):  # to leaf j of the sequence (clipped), the body itself at distance 0
        j = np.clip(j, 0, n - 1)
        return np.where(j == me, 0.0, np.hypot(x[j] - x, y[j] - y))

    for k in (8, 32):
        W = k + 1
        dk = np.maximum(tree.query(np.c_[x, y], k=k + 1)[0][:, k], 1e-300)

        def window(start):
            start = np.clip(start, 0, n - W)
            worst = np.zeros(n)
            for t in range(W):
                worst = np.maximum(worst, dist(start + t))
            return worst

        centre = window(me - W // 2)
        three = np.minimum(np.minimum(window(me - W), window(me)), centre)
        both = np.stack([np.where(np.clip(me + t, 0, n - 1) == me, np.inf, dist(me + t))
                         for t in range(-W, W + 1)], axis=1)
        union = np.partition(both, k - 1, axis=1)[:, k - 1]
        report(k, "centre", centre / dk)
        report(k, "three", three / dk)
        report(k, "union-kth", union / dk)
        m = n // 64 * 64
        s, X, Y = (a[:m].reshape(-1, 64) for a in (three, x, y))
        fixed = s.copy()
        for b in range(64):
            fixed = np.minimum(fixed, s[:, b:b + 1] + np.hypot(X - X[:, b:b + 1], Y - Y[:, b:b + 1]))
        report(k, "three+triangle", (fixed / dk[:m].reshape(-1, 64)).ravel())


if __name__ == "__main__":
    main()
