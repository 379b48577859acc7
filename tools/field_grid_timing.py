#!/usr/bin/env python3
"""The field on a grid made on the device against the same grid through compute_field
(DESIGN.md §14).

Usage (GPU box): python tools/field_grid_timing.py [reps]
C3 (theta 0.5), grids 600 x 200 and 2400 x 800 over the world (one point at the centre of each
cell).  After one warm-up of each call, `reps` alternating rounds of
  compute_field       on the host-made coordinates of the grid (upload, keys, sort, walk through
                      the order gather, copy-out): the baseline;
  compute_field_grid  the same points made by the kernel.
Every call is a fresh build of the same state.  HIP-event kernel times (field_kernel_ms,
field_grid_kernel_ms) and wall-clock call times, medians; a call without probes gives the build's
share of both calls.  Also the stats-only call (no plane comes to the host).  The two results are
compared bit for bit on the way.  Appends one JSON line to profiles/field_grid_timing.jsonl and
prints it.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "barnes-hut-n-body_amd"))
import bh_amd  # noqa: E402
from bh_amd import scenes  # noqa: E402


def med(v):
    return round(statistics.median(v), 4)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def grid(eng, reps, nx, ny):
    p = eng.params
    dx, dy = p.width_px / nx, p.height_px / ny
    g = (0.5 * dx, 0.5 * dy, dx, dy, nx, ny)
    cx = g[0] + np.arange(nx, dtype=np.float64) * dx  # the kernel's arithmetic: multiply, add
    cy = g[1] + np.arange(ny, dtype=np.float64) * dy
    px, py = (np.ascontiguousarray(a.ravel()) for a in np.meshgrid(cx, cy))
    none = np.zeros(0)
    base = eng.compute_field(px, py)  # warm-up: the probe buffers
    new = eng.compute_field_grid(*g)  # warm-up: the planes
    same = all(np.array_equal(a.view(np.int64), b.ravel().view(np.int64))
               for a, b in zip(base, new))
    eng.compute_field_grid(*g, want_accel=False, want_phi=False, want_stats=True)
    bk, bc, gk, gc, sc, bare = [], [], [], [], [], []
    # (in a loop of its own: between calls that return planes of many megabytes the host's
    # freeing of the previous planes lands on whichever call comes next)
    for _ in range(reps):
        _, ms = timed(lambda: eng.compute_field(none, none))
        bare.append(ms)
    for _ in range(reps):
        _, ms = timed(lambda: eng.compute_field(px, py))
        bc.append(ms)
        bk.append(eng.field_kernel_ms())
        _, ms = timed(lambda: eng.compute_field_grid(*g))
        gc.append(ms)
        gk.append(eng.field_grid_kernel_ms())
        _, ms = timed(lambda: eng.compute_field_grid(*g, want_accel=False, want_phi=False,
                                                     want_stats=True))
        sc.append(ms)
    r = {"nx": nx, "ny": ny, "points": nx * ny, "bit_identical": bool(same),
         "shape": list(bh_amd.field_grid_shape(nx, ny)),
         "field_kernel_ms": med(bk), "field_call_ms": med(bc),
         "grid_kernel_ms": med(gk), "grid_call_ms": med(gc),
         "grid_stats_only_call_ms": med(sc), "build_only_call_ms": med(bare)}
    r["kernel_ratio_grid_over_field"] = round(r["grid_kernel_ms"] / r["field_kernel_ms"], 4)
    r["call_ratio_grid_over_field"] = round(r["grid_call_ms"] / r["field_call_ms"], 4)
    r["field_around_kernel_ms"] = round(r["field_call_ms"] - r["build_only_call_ms"] -
                                        r["field_kernel_ms"], 4)
    r["grid_around_kernel_ms"] = round(r["grid_call_ms"] - r["build_only_call_ms"] -
                                       r["grid_kernel_ms"], 4)
    for name, v in (("field_kernel", bk), ("field_call", bc), ("grid_kernel", gk),
                    ("grid_call", gc), ("grid_stats_only_call", sc), ("build_only_call", bare)):
        r[name + "_samples"] = [round(x, 4) for x in v]
    return r


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"reps": reps, "warmup": 1}
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.compute_accelerations()  # the build's jitter, once
    out["bodies"] = eng.num_bodies()
    for nx, ny in ((600, 200), (2400, 800)):
        out[f"c3_grid_{nx}x{ny}"] = grid(eng, reps, nx, ny)
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "field_grid_timing.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
