#!/usr/bin/env python3
"""bh_render_bodies beside the read-backs it replaces.

Usage (GPU box): python tools/render_bench.py [reps] [warmup]
C3 (two colliding disks, 1e6 bodies, theta 0.5) after step(10), the default 2400 x 800 view;
medians of `reps` calls after `warmup` warm-up calls, all on one engine and one state:
  render_kernel_ms      HIP-event time of k_raster + k_resolve (pixels only / all three planes)
  render_pixels_ms      wall time of render_bodies() returning pixels only
  render_all_ms         ... returning pixels, owner and counts
  get_bodies_ms         wall time of get_bodies() (fresh arrays, and into reused arrays)
  map_bodies_ms         wall time of map_bodies() after a mirrored step(1) (measured last: it
                        steps; the step itself is outside the timed span)
  pixels_direct_ms / pixels_pinned_bounce_ms   the pixels-only call copying straight into the
                        caller's array against BH_RENDER_PINNED=1, alternating call by call
The in-wave combining of k_raster against one atomic per lane (BH_RENDER_COMBINE=0), interleaved
rounds in this one process: kernel time on the C3 state and on 1e6 bodies at one position.
Prints one JSON line.
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


def combine_ab(eng, reps, warmup, counts):
    """Kernel ms with and without the in-wave combining, alternating call by call."""
    out = {"on": [], "off": []}
    images = {}
    for r in range(warmup + reps):
        for key, env in (("on", "1"), ("off", "0")):
            os.environ["BH_RENDER_COMBINE"] = env
            images[key] = eng.render_bodies(owner=True, counts=counts)
            if r >= warmup:
                out[key].append(eng.render_kernel_ms())
    os.environ.pop("BH_RENDER_COMBINE")
    same = all(np.array_equal(a, b) for a, b in zip(images["on"], images["off"]) if a is not None)
    return {"combine_kernel_ms": med(out["on"]), "per_lane_kernel_ms": med(out["off"]),
            "combine_min_ms": round(min(out["on"]), 4), "per_lane_min_ms": round(min(out["off"]), 4),
            "same_bytes": bool(same)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    out = {"reps": reps, "warmup": warmup, "view": [2400, 800]}
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.step(10)
    out["bodies"] = eng.num_bodies()

    kms = []
    t = wall(lambda: (eng.render_bodies(), kms.append(eng.render_kernel_ms())), reps, warmup)
    out["render_pixels_ms"] = med(t)
    out["render_pixels_samples"] = [round(v, 4) for v in t]
    out["render_kernel_ms"] = med(kms[warmup:])
    buf = (np.empty((800, 2400), dtype=np.uint8), None, None)
    out["render_pixels_reused_ms"] = med(wall(lambda: eng.render_bodies(out=buf), reps, warmup))
    # pageable destination against a pinned bounce buffer + host copy, alternating
    ab = {"0": [], "1": []}
    for r in range(warmup + reps):
        for env in ("0", "1"):
            os.environ["BH_RENDER_PINNED"] = env
            t0 = time.perf_counter()
            eng.render_bodies(out=buf)
            if r >= warmup:
                ab[env].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop("BH_RENDER_PINNED")
    out["pixels_direct_ms"], out["pixels_pinned_bounce_ms"] = med(ab["0"]), med(ab["1"])
    kms = []
    t = wall(lambda: (eng.render_bodies(owner=True, counts=True),
                      kms.append(eng.render_kernel_ms())), reps, warmup)
    out["render_all_ms"] = med(t)
    out["render_all_kernel_ms"] = med(kms[warmup:])

    t = wall(eng.get_bodies, reps, warmup)
    out["get_bodies_ms"] = med(t)
    out["get_bodies_samples"] = [round(v, 4) for v in t]
    bufs = [np.empty(eng.num_bodies(), dtype=np.float64) for _ in range(5)]
    out["get_bodies_reused_ms"] = med(wall(lambda: eng.get_bodies(out=bufs), reps, warmup))
    out["pixels_over_get_bodies"] = round(out["render_pixels_ms"] / out["get_bodies_ms"], 4)

    out["c3_combine"] = combine_ab(eng, reps, warmup, counts=True)
    out["c3_combine_no_counts"] = combine_ab(eng, reps, warmup, counts=False)

    eng.set_mirror(True)
    t = []
    for r in range(warmup + reps):
        eng.step(1)
        t0 = time.perf_counter()
        eng.map_bodies()
        if r >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    out["map_bodies_ms"] = med(t)
    eng.close()

    n = 1_000_000
    z = np.zeros(n)
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(np.full(n, 1200.5), np.full(n, 400.5), z, z, np.ones(n))
    out["one_pixel_combine"] = combine_ab(eng, reps, warmup, counts=True)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
