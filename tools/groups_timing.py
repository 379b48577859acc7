#!/usr/bin/env python3
"""bh_find_groups on the C3 tree beside what a user had before it.

Usage (GPU box): python tools/groups_timing.py [reps] [limit_s]
C3 (theta 0.5), link lengths 0.05, 0.1, 0.2, 0.5 -- the C3 disk's mean separation is about 0.2, so
these span sparse to percolating -- one JSON line each.  Per link length, after one warm-up call,
`reps` interleaved rounds of
  * find_groups(link, min_members=8) with labels: groups_kernel_ms and the call,
  * the alternative: find_neighbors with lists at the same radius with the bodies as probes, on
    every k-th body where the lists of all of them together would pass 2^25 entries (the line says
    which k), and get_bodies() -- the host-side union-find that would follow is not timed,
  * a call without probes, which measures the build every call makes; the calls are also given
    net of it.
The line also holds n_groups_all, n_groups at min_members = 8, largest_count and the number of
linked pairs (from find_neighbors' counts: every body finds itself and each friend).  HIP-event
kernel times, wall-clock call times, min and median.  If one find_groups call takes longer than
limit_s (default 5) that link length gets one round, the longer ones are not run, and the
line says so.  Appends to
profiles/groups_timing.jsonl.
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

LINKS = (0.05, 0.1, 0.2, 0.5)
MIN_MEMBERS = 8


def stat(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}


def timed(eng, fn):
    """Wall-clock ms of fn(); its result is dropped and one call without probes is made before
    returning (neighbors_timing.timed: the first call after large host arrays are freed is slow
    whatever it is)."""
    t0 = time.perf_counter()
    out = fn()
    ms = (time.perf_counter() - t0) * 1e3
    del out
    eng.find_neighbors(np.zeros(0), np.zeros(0), 0.0)
    return ms


def line(eng, x, y, link, reps, limit_s):
    none = np.zeros(0)
    t0 = time.perf_counter()
    summary, _, _ = eng.find_groups(link, MIN_MEMBERS)  # warm-up: buffers, code objects
    first_call_s = time.perf_counter() - t0
    if first_call_s > limit_s:
        reps = 1  # over the limit: one round, and main() ends the sweep here
    count, _, _ = eng.find_neighbors(x, y, link)
    found = int(count.sum())
    del count
    k = max(1, -(-found // (1 << 25)))
    lx, ly = np.ascontiguousarray(x[::k]), np.ascontiguousarray(y[::k])
    res = eng.find_neighbors(lx, ly, link, lists=True)
    list_total = int(res[3][-1])
    del res
    t = {name: [] for name in ("groups_kernel", "groups_call", "neighbor_lists_kernel",
                               "neighbor_lists_call", "get_bodies", "build_only_call")}
    for _ in range(reps):
        ms = timed(eng, lambda: eng.find_groups(link, MIN_MEMBERS))
        t["groups_call"].append(ms)
        t["groups_kernel"].append(eng.groups_kernel_ms())
        ms = timed(eng, lambda: eng.find_neighbors(lx, ly, link, lists=True, cap=list_total))
        t["neighbor_lists_call"].append(ms)
        t["neighbor_lists_kernel"].append(eng.neighbors_kernel_ms())
        ms = timed(eng, eng.get_bodies)
        t["get_bodies"].append(ms)
        ms = timed(eng, lambda: eng.find_neighbors(none, none, link))
        t["build_only_call"].append(ms)
    out = {"link": link, "min_members": MIN_MEMBERS, "n_in_tree": summary.n_in_tree,
           "n_groups_all": summary.n_groups_all, "n_groups": summary.n_groups,
           "largest_count": summary.largest_count,
           "linked_pairs": (found - summary.n_in_tree) // 2,
           "mean_friends": round((found - summary.n_in_tree) / max(summary.n_in_tree, 1), 3),
           "first_call_s": round(first_call_s, 4), "rounds": reps,
           "neighbor_lists_every_kth_body": k, "neighbor_lists_probes": len(lx),
           "neighbor_lists_entries": list_total}
    out.update({f"{name}_ms": stat(v) for name, v in t.items()})
    b = out["build_only_call_ms"]["median"]
    # find_groups as Engine.find_groups makes it: a sizing call and the call itself, two builds
    out["groups_call_net_of_builds_ms"] = round(out["groups_call_ms"]["median"] - 2 * b, 4)
    out["neighbor_lists_call_net_of_build_ms"] = round(
        out["neighbor_lists_call_ms"]["median"] - b, 4)
    return out, first_call_s


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    limit_s = float(sys.argv[2]) if len(sys.argv) > 2 else 5.0
    head = os.environ.get("BH_TIMING_HEAD")  # (a copy of the tree that is no git checkout)
    if not head:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                  capture_output=True, text=True).stdout.strip() or None
        except OSError:
            head = None
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.compute_accelerations()  # the build's jitter, if any, once
    x, y, _, _, _ = eng.get_bodies()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "groups_timing.jsonl")
    for i, link in enumerate(LINKS):
        out = {"scene": "c3", "bodies": len(x), "reps": reps, "warmup": 1, "head": head}
        got, first_call_s = line(eng, x, y, link, reps, limit_s)
        out.update(got)
        stop = first_call_s > limit_s and i + 1 < len(LINKS)
        if stop:
            out["sweep_stopped"] = {"limit_s": limit_s, "not_run": list(LINKS[i + 1:])}
        text = json.dumps(out)
        with open(path, "a") as f:
            f.write(text + "\n")
        print(text, flush=True)
        if stop:
            break
    eng.close()


if __name__ == "__main__":
    main()
