#!/usr/bin/env python3
"""Tracer walk against the field kernel, and the step with and without tracers.

Usage (GPU box): python tools/tracers_timing.py [reps] [steps]
C3 (theta 0.5), tracers = the 10^6 bodies' own start positions and velocities.
 1. kernel: `reps` rounds of compute_field() at the tracers' current positions (field_kernel_ms:
    k_field, with phi and its stores) and then one profiled step() (tracer_kernel_ms: the average
    of the step's two k_tracer_step launches, the first of them on that same tree at those same
    points), after one warm-up round.
 2. step: `reps` alternating rounds of one step(steps) call (default 64) without tracers, with the
    first 10^5 and with all 10^6 of them, profiling off; wall-clock ms per step.  The bodies are the
    same in all three (tracers exert nothing), so the three share one drifting state.
R, the steps between re-orderings of the tracers' lane map, is a compile-time constant of the
library (reported here from tracer_launch_shape): a sweep runs this tool once per build, with
BH_ENGINE_LIB naming the library.  Medians and every sample; appends one JSON line to
profiles/tracers_timing.jsonl and prints it.
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


def kernels(eng, reps):
    eng.set_profiling(True)
    fld, trc = [], []
    for r in range(reps + 1):  # (round 0 warms up: the probe buffers, both kernels)
        tx, ty, _, _ = eng.get_tracers()
        eng.compute_field(tx, ty, want_accel=True, want_phi=True)
        f = eng.field_kernel_ms()
        eng.step(1)
        t, launches = eng.tracer_kernel_ms()
        assert launches == 2
        if r:
            fld.append(f)
            trc.append(t)
    eng.set_profiling(False)
    f, t = med(fld), med(trc)
    return {"tracers": eng.num_tracers(), "field_kernel_ms": f, "tracer_kernel_ms": t,
            "tracer_over_field": round(t / f, 4), "field_samples": [round(v, 4) for v in fld],
            "tracer_samples": [round(v, 4) for v in trc]}


def steps(eng, tr, reps, k):
    none = tuple(np.zeros(0) for _ in range(4))
    cases = (("no_tracers", none), ("tracers_1e5", tuple(a[:100_000] for a in tr)),
             ("tracers_1e6", tr))
    ms = {name: [] for name, _ in cases}
    for r in range(reps + 1):  # (round 0 warms up every shape)
        for name, t in cases:
            eng.set_tracers(*t)
            t0 = time.perf_counter()
            eng.step(k)
            dt = (time.perf_counter() - t0) * 1e3 / k
            if r:
                ms[name].append(dt)
    out = {"steps_per_call": k}
    for name, _ in cases:
        out[name + "_ms_per_step"] = med(ms[name])
        out[name + "_samples"] = [round(v, 4) for v in ms[name]]
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    x, y, vx, vy, m = scenes.config_scene("c3")
    tr = tuple(np.ascontiguousarray(a) for a in (x, y, vx, vy))
    bpw, wpb, R = bh_amd.tracer_launch_shape(len(x))
    out = {"reps": reps, "warmup": 1, "library": os.path.relpath(bh_amd.LIB_PATH, ROOT),
           "tracers_per_wave": bpw, "waves_per_group": wpb, "reorder_steps": R}
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(x, y, vx, vy, m)
    eng.set_tracers(*tr)
    out["c3_kernel"] = kernels(eng, reps)
    out["c3_step"] = steps(eng, tr, reps, k)
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tracers_timing.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
