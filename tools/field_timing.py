#!/usr/bin/env python3
"""Field kernel against the force and potential kernels on the same tree state.

Usage (GPU box): python tools/field_timing.py [reps]
C3 (theta 0.5), probes = the bodies' own positions and masses: after one warm-up call of each,
`reps` alternating rounds of a plain compute_accelerations() (traverse_kernel_ms: k_traverse),
compute_potential() (potential_kernel_ms) and compute_field() (field_kernel_ms), every call on a
fresh build of the same state; once right after the reset and once after 5 steps (the Hilbert
lane map live for the two body walks; the probes are always in the order of their own Morton
keys).  Then a 600 x 200 grid over the world (120 000 probes of unit mass) on the C3 tree: the
kernel, the whole call, a call without probes (the build alone) and what is left around the
kernel -- upload, keys, sort, copy-out.  HIP-event kernel times, wall-clock call times, medians.
Appends one JSON line to profiles/field_timing.jsonl and prints it.
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


def rounds(eng, reps):
    eng.set_profiling(True)
    eng.compute_accelerations()  # warm-up (and the build's jitter, once)
    eng.compute_potential()
    x, y, _, _, m = eng.get_bodies()
    eng.compute_field(x, y, m)
    trav, pot, fld = [], [], []
    for _ in range(reps):
        eng.compute_accelerations()
        trav.append(eng.traverse_kernel_ms()[0])
        eng.compute_potential()
        pot.append(eng.potential_kernel_ms())
        eng.compute_field(x, y, m)
        fld.append(eng.field_kernel_ms())
    t, p, f = med(trav), med(pot), med(fld)
    return {"bodies": len(x), "traverse_kernel_ms": t, "potential_kernel_ms": p,
            "field_kernel_ms": f, "field_over_traverse": round(f / t, 4),
            "field_over_sum": round(f / (t + p), 4),
            "traverse_samples": [round(v, 4) for v in trav],
            "potential_samples": [round(v, 4) for v in pot],
            "field_samples": [round(v, 4) for v in fld]}


def grid(eng, reps, nx=600, ny=200):
    p = eng.params
    gx = (np.arange(nx) + 0.5) * (p.width_px / nx)
    gy = (np.arange(ny) + 0.5) * (p.height_px / ny)
    px, py = (np.ascontiguousarray(a.ravel()) for a in np.meshgrid(gx, gy))
    none = np.zeros(0)
    eng.compute_field(px, py)  # warm-up: the probe buffers
    kern, call, bare = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.compute_field(px, py)
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(eng.field_kernel_ms())
        t0 = time.perf_counter()
        eng.compute_field(none, none)
        bare.append((time.perf_counter() - t0) * 1e3)
    k, c, b = med(kern), med(call), med(bare)
    return {"probes": len(px), "field_kernel_ms": k, "call_ms": c, "build_only_call_ms": b,
            "around_kernel_ms": round(c - b - k, 4), "kernel_samples": [round(v, 4) for v in kern],
            "call_samples": [round(v, 4) for v in call],
            "build_only_samples": [round(v, 4) for v in bare]}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"reps": reps, "warmup": 1}
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    out["c3_after_reset"] = rounds(eng, reps)
    eng.set_profiling(False)
    out["c3_grid_600x200"] = grid(eng, reps)
    eng.step(5)
    out["c3_after_5_steps"] = rounds(eng, reps)
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "field_timing.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
