#!/usr/bin/env python3
"""bh_find_knn / bh_find_knn_bodies beside the radius walk given the answer.

Usage (GPU box): python tools/knn_timing.py [reps]
C3 (theta 0.5).  After one warm-up call of each, `reps` interleaved rounds of
  * find_knn_bodies at k = 1, 8, 32, 64: knn_kernel_ms and the call,
  * find_knn with the 10^6 body positions as probes at k = 8 and k = 32: kernel and call,
  * find_neighbors counts-only on the same probes with r = the median of the measured sqrt(d2_k)
    of find_knn at k = 8 and at k = 32: the radius walk given the answer in advance, the floor the
    seed is judged against,
  * find_knn once more with that radius as r_max: the k-nearest walk given the same answer, so
    that what the lists cost and what the seed costs can be told apart,
  * compute_field on the same probes: field_kernel_ms, the yardstick,
  * get_bodies().
Every call builds the tree anew (C3 has no jitter cell, so the state does not move); a call
without probes measures that build, and the calls are also given net of it.  HIP-event kernel
times, wall-clock call times, min and median; between two timed calls the results are freed and
one untimed call without probes is made (see timed()).  Appends one JSON line to
profiles/knn_timing.jsonl.
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

BODIES_K = (1, 8, 32, 64)
PROBES_K = (8, 32)


def stat(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def timed(eng, fn):
    """Wall-clock ms of fn().  Its result is dropped and one call without probes is made before
    returning: the first engine call after large host arrays are freed takes 20-30 ms on this
    stack whatever it is, and that must not land in the next measurement
    (tools/neighbors_timing.py)."""
    t0 = time.perf_counter()
    out = fn()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    eng.find_neighbors(np.zeros(0), np.zeros(0), 0.0)
    return ms


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
    x, y, _, _, _ = eng.get_bodies()
    none = np.zeros(0)
    out = {"scene": "c3", "bodies": len(x), "reps": reps, "warmup": 1, "head": head}
    # warm-up (buffers, code objects), and the radii the radius walk is given
    radius = {}
    for k in BODIES_K:
        _, d2, found = eng.find_knn_bodies(k)
        out[f"bodies_k{k}_median_dk"] = round(float(np.sqrt(np.median(d2[:, k - 1]))), 4)
        del d2, found
    for k in PROBES_K:
        _, d2, _ = eng.find_knn(x, y, k)
        radius[k] = float(np.sqrt(np.median(d2[:, k - 1])))
        out[f"probes_k{k}_median_dk"] = round(radius[k], 4)
        del d2
        count, _, _ = eng.find_neighbors(x, y, radius[k])
        out[f"radius_k{k}_mean_count"] = round(float(count.mean()), 2)
        del count
    eng.compute_field(x, y)
    names = [f"bodies_k{k}" for k in BODIES_K] + [f"probes_k{k}" for k in PROBES_K] + \
            [f"radius_k{k}" for k in PROBES_K] + [f"capped_k{k}" for k in PROBES_K] + ["field"]
    t = {f"{n}_{w}": [] for n in names for w in ("kernel", "call")}
    t["get_bodies"], t["build_only_call"] = [], []
    for _ in range(reps):
        for k in BODIES_K:
            t[f"bodies_k{k}_call"].append(timed(eng, lambda: eng.find_knn_bodies(k)))
            t[f"bodies_k{k}_kernel"].append(eng.knn_kernel_ms())
        for k in PROBES_K:
            t[f"probes_k{k}_call"].append(timed(eng, lambda: eng.find_knn(x, y, k)))
            t[f"probes_k{k}_kernel"].append(eng.knn_kernel_ms())
            t[f"radius_k{k}_call"].append(timed(eng, lambda: eng.find_neighbors(x, y, radius[k])))
            t[f"radius_k{k}_kernel"].append(eng.neighbors_kernel_ms())
            t[f"capped_k{k}_call"].append(timed(eng, lambda: eng.find_knn(x, y, k, radius[k])))
            t[f"capped_k{k}_kernel"].append(eng.knn_kernel_ms())
        t["field_call"].append(timed(eng, lambda: eng.compute_field(x, y)))
        t["field_kernel"].append(eng.field_kernel_ms())
        t["get_bodies"].append(timed(eng, eng.get_bodies))
        t["build_only_call"].append(timed(eng, lambda: eng.find_neighbors(none, none, 0.0)))
    out.update({f"{name}_ms": stat(v) for name, v in t.items()})
    b = out["build_only_call_ms"]["median"]
    for n in names:
        out[f"{n}_call_net_of_build_ms"] = round(out[f"{n}_call_ms"]["median"] - b, 4)
    for k in PROBES_K:
        out[f"probes_k{k}_over_radius_kernel"] = round(
            out[f"probes_k{k}_kernel_ms"]["median"] / out[f"radius_k{k}_kernel_ms"]["median"], 4)
        out[f"capped_k{k}_over_radius_kernel"] = round(
            out[f"capped_k{k}_kernel_ms"]["median"] / out[f"radius_k{k}_kernel_ms"]["median"], 4)
    out["bodies_k8_over_radius_k8_kernel"] = round(
        out["bodies_k8_kernel_ms"]["median"] / out["radius_k8_kernel_ms"]["median"], 4)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    text = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "knn_timing.jsonl"), "a") as f:
        f.write(text + "\n")
    print(text, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
