#!/usr/bin/env python3
"""bh_find_neighbors against the field walk on the same probes and tree.

Usage (GPU box): python tools/neighbors_timing.py [reps]
C3 (theta 0.5), probes = the 10^6 bodies' own positions, r = merge_min_dist (8) and r = 50, one
JSON line each.  After one warm-up call of each, `reps` interleaved rounds of
  * find_neighbors counts-only (count, nearest, d2_nearest): neighbors_kernel_ms and the call,
  * find_neighbors with lists, on every k-th probe where the 10^6 lists together would pass
    2^25 entries (the line says which k, and the total for all probes),
  * compute_field on the same probes: field_kernel_ms, the yardstick,
  * get_bodies(), the copy the call replaces,
  * one probe at the heaviest body, nearest alone (the pick): kernel and call.
Every call builds the tree anew (C3 has no jitter cell, so the state does not move); a call
without probes measures that build, and the calls are also given net of it.  HIP-event kernel
times, wall-clock call times, min and median; between two timed calls the results are freed and
one untimed call without probes is made (see timed()).  Appends to
profiles/neighbors_timing.jsonl.
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


def stat(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def timed(eng, fn):
    """Wall-clock ms of fn().  Its result is dropped and one call without probes is made before
    returning: the first engine call after large host arrays are freed takes 20-30 ms on this
    stack whatever it is (a get_bodies() result freed before a build-only query: 22 ms against
    0.26 ms), and that must not land in the next measurement."""
    t0 = time.perf_counter()
    out = fn()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    eng.find_neighbors(np.zeros(0), np.zeros(0), 0.0)
    return ms


def line(eng, x, y, r, reps, heavy):
    none = np.zeros(0)
    count, _, _ = eng.find_neighbors(x, y, r)  # warm-up: buffers, code objects
    total = int(count.sum())
    k = max(1, -(-total // (1 << 25)))
    lx, ly = np.ascontiguousarray(x[::k]), np.ascontiguousarray(y[::k])
    res = eng.find_neighbors(lx, ly, r, lists=True)
    list_total = int(res[3][-1])
    del res
    eng.compute_field(x, y)
    eng.find_neighbors(x[heavy:heavy + 1], y[heavy:heavy + 1], r, counts=False)
    t = {k_: [] for k_ in ("count_kernel", "count_call", "lists_kernel", "lists_call",
                           "field_kernel", "field_call", "get_bodies", "pick_kernel",
                           "pick_call", "build_only_call")}
    for _ in range(reps):
        ms = timed(eng, lambda: eng.find_neighbors(x, y, r))
        t["count_call"].append(ms)
        t["count_kernel"].append(eng.neighbors_kernel_ms())
        ms = timed(eng, lambda: eng.find_neighbors(lx, ly, r, lists=True, cap=list_total))
        t["lists_call"].append(ms)
        t["lists_kernel"].append(eng.neighbors_kernel_ms())
        ms = timed(eng, lambda: eng.compute_field(x, y))
        t["field_call"].append(ms)
        t["field_kernel"].append(eng.field_kernel_ms())
        ms = timed(eng, eng.get_bodies)
        t["get_bodies"].append(ms)
        ms = timed(eng, lambda: eng.find_neighbors(x[heavy:heavy + 1], y[heavy:heavy + 1], r,
                                                 counts=False))
        t["pick_call"].append(ms)
        t["pick_kernel"].append(eng.neighbors_kernel_ms())
        ms = timed(eng, lambda: eng.find_neighbors(none, none, r))
        t["build_only_call"].append(ms)
    out = {"r": r, "probes": len(x), "neighbours_in_all": total, "mean_count": round(total / len(x), 2),
           "lists_every_kth_probe": k, "lists_probes": len(lx), "lists_entries": list_total}
    out.update({f"{name}_ms": stat(v) for name, v in t.items()})
    b = out["build_only_call_ms"]["median"]
    for name in ("count", "lists", "field", "pick"):
        out[f"{name}_call_net_of_build_ms"] = round(out[f"{name}_call_ms"]["median"] - b, 4)
    out["count_over_field_kernel"] = round(out["count_kernel_ms"]["median"] /
                                           out["field_kernel_ms"]["median"], 4)
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    head = os.environ.get("BH_TIMING_HEAD")  # (a copy of the tree that is no git checkout)
    if not head:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                  capture_output=True, text=True).stdout.strip() or None
        except OSError:
            head = None
    params = bh_amd.default_params(theta=0.5)
    eng = bh_amd.Engine(params, device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.compute_accelerations()  # the build's jitter, if any, once
    x, y, _, _, m = eng.get_bodies()
    heavy = int(np.argmax(m))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for r in (float(params.merge_min_dist), 50.0):
        out = {"scene": "c3", "bodies": len(x), "reps": reps, "warmup": 1, "head": head}
        out.update(line(eng, x, y, r, reps, heavy))
        text = json.dumps(out)
        with open(os.path.join(ROOT, "profiles", "neighbors_timing.jsonl"), "a") as f:
            f.write(text + "\n")
        print(text, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
