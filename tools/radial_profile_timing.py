#!/usr/bin/env python3
"""bh_compute_radial_profile on C3 beside what a user had before it.

Usage (GPU box): python tools/radial_profile_timing.py [out.jsonl] [reps]
C3 (theta 0.5) after 20 steps, the profile about (1200, 400) with linear bins over [0, 1200]:
64 bins, 1 bin and 4096 bins, one JSON line each.  Per bin count, after 3 warm-up calls, `reps`
(default 20) interleaved rounds of
  * Engine.radial_profile: radial_profile_kernel_ms (HIP events, staging to last emit kernel) and
    the wall time of the Python call (it ends in a device synchronise and the copy-out),
  * the same call on a subset (every second body),
  * the copy-out route: get_bodies() plus a vectorised numpy binning of the same seven sums
    (np.searchsorted and np.bincount with weights), the two parts timed apart,
  * diagnostics(potential=False): the floor of a no-build reduction over the same staging.
Medians and minima.  Appends to profiles/radial_profile_timing.jsonl unless told otherwise.
"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "barnes-hut-n-body_amd"))
import bh_amd  # noqa: E402
from bh_amd import scenes  # noqa: E402

CENTRE = (1200.0, 400.0)
BINS = (64, 1, 4096)
WARMUP = 3


def stat(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def host_binning(arrs, edges):
    """The seven sums and the counts by bin with numpy (pairwise sums: not the call's bits)."""
    x, y, vx, vy, m = arrs
    dx, dy = x - CENTRE[0], y - CENTRE[1]
    R = np.sqrt(dx * dx + dy * dy)
    with np.errstate(all="ignore"):
        vr = np.where(R == 0.0, 0.0, (dx * vx + dy * vy) / R)
        w = dx * vy - dy * vx
        vt = np.where(R == 0.0, 0.0, w / R)
    k = np.searchsorted(edges, R, side="right") - 1
    ok = (k >= 0) & (k < len(edges) - 1)
    k = k[ok]
    nb = len(edges) - 1
    out = [np.bincount(k, minlength=nb)]
    for t in (m, m * R, m * vr, m * vt, m * vr * vr, m * vt * vt, m * w):
        out.append(np.bincount(k, weights=t[ok], minlength=nb))
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles",
                                                                  "radial_profile_timing.jsonl")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.step(20)
    n = eng.num_bodies()
    half = np.arange(0, n, 2, dtype=np.int64)
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                              capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    for n_bin in BINS:
        edges = bh_amd.radial_edges(0.0, 1200.0, n_bin)
        for _ in range(WARMUP):
            p = eng.radial_profile(*CENTRE, edges)
            eng.radial_profile(*CENTRE, edges, subset=half)
            host_binning(eng.get_bodies(), edges)
            eng.diagnostics(potential=False)
        t = {k: [] for k in ("kernel", "call", "kernel_subset", "call_subset", "get_bodies",
                             "numpy_binning", "diagnostics")}
        for _ in range(reps):
            ms, p = wall(lambda: eng.radial_profile(*CENTRE, edges))
            t["call"].append(ms)
            t["kernel"].append(eng.radial_profile_kernel_ms())
            ms, _ = wall(lambda: eng.radial_profile(*CENTRE, edges, subset=half))
            t["call_subset"].append(ms)
            t["kernel_subset"].append(eng.radial_profile_kernel_ms())
            ms, arrs = wall(eng.get_bodies)
            t["get_bodies"].append(ms)
            ms, host = wall(lambda: host_binning(arrs, edges))
            t["numpy_binning"].append(ms)
            ms, _ = wall(lambda: eng.diagnostics(potential=False))
            t["diagnostics"].append(ms)
        assert np.array_equal(host[0], p.count), "the host binning counts differ from the call's"
        rel = np.abs(host[1] - p.mass).max() / max(np.abs(p.mass).max(), 1e-300)
        line = {"scene": "c3 after 20 steps", "n": n, "n_bin": n_bin, "reps": reps,
                "warmup": WARMUP, "head": head, "n_binned": p.summary.n_binned,
                "n_outer": p.summary.n_outer, "mass_rel_diff_vs_numpy": float(rel),
                "ms": {k: stat(v) for k, v in t.items()}}
        print(json.dumps(line), flush=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
