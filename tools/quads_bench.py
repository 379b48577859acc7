#!/usr/bin/env python3
"""bh_render_quads beside the bh_get_quads it replaces.

Usage (GPU box): python tools/quads_bench.py [reps] [warmup] >> profiles/quads_bench.jsonl
C3 (two colliding disks, 1e6 bodies, theta 0.5) after step(10), the default 2400 x 800 view;
medians of `reps` calls after `warmup` warm-up calls, all on one engine and one state (lastTree
of the call; neither call changes it):
  render_quads_ms         wall time of render_quads() returning the count plane
  render_quads_kernel_ms  HIP-event time of its three kernels (cells, row scan, column scan)
  count_only_ms           wall time of render_quads(lines=None); count_only_kernel_ms its kernel
  get_quads_ms            wall time of get_quads() (the sizing call and the fetching call, as
                          every caller of bh_get_quads makes them); get_quads_one_walk_ms the
                          fetching call alone into arrays of the known size
  *_variants              how one-pixel cells are drawn, alternating call by call, kernel and wall
                          time: `combine` (the default: +2 per cell, equal pixels summed in the
                          lane and the wave first), `direct` (BH_QUADS_COMBINE=0: one atomic per
                          cell), `difference` (BH_QUADS_DIRECT=0: through the difference planes) --
                          at the default view, at zoom 10 and with the whole root in 731 x 733
Prints one JSON line.
"""
import ctypes
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


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def med(v):
    return round(statistics.median(v), 4)


VARIANTS = {  # how one-pixel cells are drawn: (BH_QUADS_DIRECT, BH_QUADS_COMBINE)
    "combine": ("1", "1"),     # +2 per cell, runs of equal pixels summed in the lane and the wave
    "direct": ("1", "0"),      # +2 per cell, one atomic each
    "difference": ("0", "0"),  # through the difference planes, as every other cell
}


def variants_ab(eng, reps, warmup, **view):
    """Kernel and wall ms of the three variants, alternating call by call."""
    kern = {k: [] for k in VARIANTS}
    walls = {k: [] for k in VARIANTS}
    images = {}
    for r in range(warmup + reps):
        for key, (direct, combine) in VARIANTS.items():
            os.environ["BH_QUADS_DIRECT"], os.environ["BH_QUADS_COMBINE"] = direct, combine
            t0 = time.perf_counter()
            images[key] = eng.render_quads(**view)[0]
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                walls[key].append(dt)
                kern[key].append(eng.render_quads_kernel_ms())
    os.environ.pop("BH_QUADS_DIRECT")
    os.environ.pop("BH_QUADS_COMBINE")
    out = {"same_bytes": all(bool(np.array_equal(images["combine"], images[k])) for k in VARIANTS)}
    for k in VARIANTS:
        out[k] = {"kernel_ms": med(kern[k]), "kernel_min_ms": round(min(kern[k]), 4),
                  "wall_ms": med(walls[k])}
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    out = {"reps": reps, "warmup": warmup, "view": [2400, 800]}
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.step(10)
    out["bodies"] = eng.num_bodies()

    kms = []
    t = wall(lambda: (eng.render_quads(), kms.append(eng.render_quads_kernel_ms())), reps, warmup)
    out["render_quads_ms"] = med(t)
    out["render_quads_samples"] = [round(v, 4) for v in t]
    out["render_quads_kernel_ms"] = med(kms[warmup:])
    lines, cells = eng.render_quads()
    out["cells"] = cells
    out["lit_pixels"] = int(np.count_nonzero(lines))
    out["max_count"] = int(lines.max())
    buf = np.empty((800, 2400), dtype=np.uint32)
    out["render_quads_reused_ms"] = med(wall(lambda: eng.render_quads(out=buf), reps, warmup))
    kms = []
    t = wall(lambda: (eng.render_quads(lines=None), kms.append(eng.render_quads_kernel_ms())),
             reps, warmup)
    out["count_only_ms"] = med(t)
    out["count_only_kernel_ms"] = med(kms[warmup:])

    t = wall(eng.get_quads, reps, warmup)
    out["get_quads_ms"] = med(t)
    out["get_quads_samples"] = [round(v, 4) for v in t]
    assert len(eng.get_quads()[0]) == cells
    q = [np.empty(cells, dtype=np.float64) for _ in range(3)]
    need = ctypes.c_int64(0)
    dp = ctypes.POINTER(ctypes.c_double)

    def one_walk():
        rc = eng._lib.bh_get_quads(eng._h, *[a.ctypes.data_as(dp) for a in q], cells,
                                   ctypes.byref(need))
        assert rc == bh_amd.BH_OK and need.value == cells

    out["get_quads_one_walk_ms"] = med(wall(one_walk, reps, warmup))
    out["render_over_get_quads"] = round(out["render_quads_ms"] / out["get_quads_ms"], 5)
    out["render_over_one_walk"] = round(out["render_quads_ms"] / out["get_quads_one_walk_ms"], 5)

    out["c3_variants"] = variants_ab(eng, reps, warmup)
    # the panel's largest zoom on the first disk's centre, and the whole root in one small view
    out["zoom10_variants"] = variants_ab(eng, reps, warmup, view_x=1150.0, view_y=380.0, zoom=10.0)
    out["whole_root_variants"] = variants_ab(eng, reps, warmup, view_x=-2.0, view_y=-802.0,
                                             zoom=0.3, width=731, height=733)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
