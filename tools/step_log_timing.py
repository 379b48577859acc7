#!/usr/bin/env python3
"""The step log's cost, and the route a user had without it.

Usage (GPU box): python tools/step_log_timing.py [reps] [steps] [--parent-lib PATH]
C3 and C2 (theta 0.5), `steps`-step calls (default 20), one warm-up round, then `reps` interleaved
rounds; medians and every sample.
 a. log off against another build of the library (--parent-lib: the parent commit's
    libbh_engine.so; skipped without it): C3 wall-clock ms per step, each round one fresh child
    process per library (a process loads one library), the two alternating.
 b. log on against log off on ONE engine, the log switched between calls (it changes nothing of
    the simulation, so both share one drifting state): wall-clock ms per step with profiling off;
    then, profiled, the kick-only walk with and without the potential (every second entry of
    traverse_kernel_samples from the last: every step's second walk), the log's staging and reduction
    (step_log_kernel_ms), and bh_compute_potential's kernel on the tree the call left
    (potential_kernel_ms) -- the walk the fusion saves.
 c. the route without the log: one-step calls with diagnostics(potential=True) after each,
    against one-step calls with the log on, wall-clock ms per step.
Appends one JSON line to profiles/step_log_timing.jsonl and prints it.
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "barnes-hut-n-body_amd"))
import bh_amd  # noqa: E402  (loads no library before its first use)


def med(v):
    return round(statistics.median(v), 4)


def rnd(v):
    return [round(u, 4) for u in v]


def timed(eng, k):
    t0 = time.perf_counter()
    eng.step(k)
    return (time.perf_counter() - t0) * 1e3 / k


def child(path, scene, k, calls):
    """--child: the bodies saved in `scene` on the library at `path`, log off, one warm-up call
    and `calls` timed ones; prints their ms per step.  `path` is the only build of the library this
    process loads -- the binding loads its own with RTLD_GLOBAL, and a second build loaded beside
    it would bind its own symbols to the first one's -- and it is driven through the few entry
    points every build has."""
    import ctypes
    z = np.load(scene)
    arrs = tuple(np.ascontiguousarray(z[f], dtype=np.float64) for f in ("x", "y", "vx", "vy", "m"))
    lib = ctypes.CDLL(path)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.bh_create.argtypes = [ctypes.POINTER(bh_amd.BhParams), ctypes.c_int,
                              ctypes.POINTER(ctypes.c_void_p)]
    lib.bh_reset_bodies.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [dp] * 5
    lib.bh_step.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.bh_destroy.argtypes = [ctypes.c_void_p]
    lib.bh_destroy.restype = None
    lib.bh_default_params.argtypes = [ctypes.POINTER(bh_amd.BhParams)]
    lib.bh_default_params.restype = None
    h = ctypes.c_void_p()
    p = bh_amd.BhParams()
    lib.bh_default_params(ctypes.byref(p))
    p.theta = 0.5
    assert lib.bh_create(ctypes.byref(p), 0, ctypes.byref(h)) == 0
    assert lib.bh_reset_bodies(h, len(arrs[0]), *[a.ctypes.data_as(dp) for a in arrs]) == 0
    assert lib.bh_step(h, k) == 0
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        assert lib.bh_step(h, k) == 0
        ms.append((time.perf_counter() - t0) * 1e3 / k)
    print(json.dumps(ms))
    lib.bh_destroy(h)


def against_parent(parent, reps, k):
    from bh_amd import scenes
    libs = (("parent", os.path.abspath(parent)), ("this", bh_amd.LIB_PATH))
    ms = {name: [] for name, _ in libs}
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "c3.npz")
        np.savez(scene, **dict(zip(("x", "y", "vx", "vy", "m"), scenes.config_scene("c3"))))
        for r in range(reps + 1):  # (round 0 warms up the machine)
            for name, lib in libs:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib,
                                      scene, str(k), "3"], check=True, capture_output=True,
                                     text=True, timeout=300)
                if r:
                    ms[name].append(
                        statistics.median(json.loads(out.stdout.strip().splitlines()[-1])))
    return {"steps_per_call": k, "parent_ms_per_step": med(ms["parent"]),
            "this_ms_per_step": med(ms["this"]), "parent_samples": rnd(ms["parent"]),
            "this_samples": rnd(ms["this"]),
            "spread_parent": round(max(ms["parent"]) - min(ms["parent"]), 4),
            "spread_this": round(max(ms["this"]) - min(ms["this"]), 4)}


def log_on_off(eng, reps, k):
    wall = {"off": [], "on": []}
    for r in range(reps + 1):
        for name in ("off", "on"):
            eng.set_step_log(64 if name == "on" else 0)
            dt = timed(eng, k)
            if r:
                wall[name].append(dt)
    eng.set_profiling(True)
    kick = {"off": [], "on": []}
    stage, pot = [], []
    for r in range(reps + 1):
        for name in ("off", "on"):
            eng.set_step_log(64 if name == "on" else 0)
            eng.step(k)
            # every step's kick-only walk: each second sample, counted from the end (a call that
            # starts on the tree the previous one built ahead has no interval for its first walk)
            second = eng.traverse_kernel_samples()[::-1][::2]
            assert len(second) == k
            if name == "on":
                ms, launches = eng.step_log_kernel_ms()
                assert launches == k
            if r:
                kick[name].append(statistics.mean(second))
                if name == "on":
                    stage.append(ms)
        eng.compute_potential()  # on the tree the call built ahead
        if r:
            pot.append(eng.potential_kernel_ms())
    eng.set_profiling(False)
    eng.set_step_log(0)
    added = med(kick["on"]) - med(kick["off"])
    return {"steps_per_call": k, "off_ms_per_step": med(wall["off"]),
            "on_ms_per_step": med(wall["on"]), "off_samples": rnd(wall["off"]),
            "on_samples": rnd(wall["on"]), "kick_walk_ms": med(kick["off"]),
            "kick_walk_pot_ms": med(kick["on"]), "kick_walk_added_ms": round(added, 4),
            "kick_walk_samples": rnd(kick["off"]), "kick_walk_pot_samples": rnd(kick["on"]),
            "staging_reduction_ms": med(stage), "staging_reduction_samples": rnd(stage),
            "potential_kernel_ms": med(pot), "potential_kernel_samples": rnd(pot)}


def one_step_routes(eng, reps, k):
    ms = {"step1_diagnostics": [], "step1_log": []}
    for r in range(reps + 1):
        eng.set_step_log(0)
        t0 = time.perf_counter()
        for _ in range(k):
            eng.step(1)
            eng.diagnostics(potential=True)
        a = (time.perf_counter() - t0) * 1e3 / k
        eng.set_step_log(64)
        t0 = time.perf_counter()
        for _ in range(k):
            eng.step(1)
        eng.get_step_log()
        b = (time.perf_counter() - t0) * 1e3 / k
        if r:
            ms["step1_diagnostics"].append(a)
            ms["step1_log"].append(b)
    eng.set_step_log(0)
    return {"steps": k, "step1_diagnostics_ms_per_step": med(ms["step1_diagnostics"]),
            "step1_log_ms_per_step": med(ms["step1_log"]),
            "step1_diagnostics_samples": rnd(ms["step1_diagnostics"]),
            "step1_log_samples": rnd(ms["step1_log"])}


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], args[2], int(args[3]), int(args[4]))
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 5
    k = int(args[1]) if len(args) > 1 else 20
    out = {"reps": reps, "warmup": 1, "library": os.path.relpath(bh_amd.LIB_PATH, ROOT)}
    if parent:
        out["c3_log_off_against_parent"] = against_parent(parent, reps, k)
    from bh_amd import scenes
    for name in ("c3", "c2"):
        eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
        eng.reset_bodies(*scenes.config_scene(name))
        eng.step(k)  # (the first call's allocations and first build)
        out[name + "_call"] = log_on_off(eng, reps, k)
        out[name + "_one_step_routes"] = one_step_routes(eng, reps, k)
        eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "step_log_timing.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
