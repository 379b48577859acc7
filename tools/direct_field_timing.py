#!/usr/bin/env python3
"""The all-pairs target kernel (k_direct_targets) timed where it is used.

Usage (GPU box): python tools/direct_field_timing.py [reps] [label]
(a) C3 at theta 0.5: force_error(sample=4096) -- the whole call, the all-pairs kernel
    (direct_field_kernel_ms) and the summary the call returned: what an on-demand accuracy
    read-out costs (one wave walks 10^6 leaves in order for every 64 samples).
(b) C5 (262 144 bodies), the first 120 000 bodies' positions as probes: compute_field_direct on
    a theta = 0.5 engine beside compute_field on a theta = 0 engine (the walk, field_kernel_ms).
(c) The same tree with the first 4096 of those probes (the small-count launch shape), and a
    sweep of probe counts around the switch between the two launch shapes.
Medians of `reps` (default 5) after 1 warm-up, from the HIP-event kernel times; call times are
wall clock.  `label` (optional) names the library build (BH_ENGINE_LIB) in the record.
Appends one JSON line to profiles/direct_field_timing.jsonl and prints it.
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

SWEEP = (4096, 16384, 32768, 32769, 65536, 98304, 131072, 262144)


def med(v):
    return round(statistics.median(v), 4)


def force_error_c3(reps):
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    eng.force_error(sample=4096)  # warm-up: the buffers, the build's jitter
    call, kern, bare = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fe = eng.force_error(sample=4096)
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(eng.direct_field_kernel_ms())
        t0 = time.perf_counter()
        eng.force_error(np.zeros(0, dtype=np.int64))  # the build and the evaluation alone
        bare.append((time.perf_counter() - t0) * 1e3)
    n = eng.num_bodies()
    eng.close()
    return {"bodies": n, "theta": 0.5, "samples": fe.n_sample,
            "shape": bh_amd.direct_field_shape(fe.n_sample), "call_ms": med(call),
            "direct_kernel_ms": med(kern), "call_without_samples_ms": med(bare),
            "n_used": fe.n_used, "worst": fe.worst, "max_rel": fe.max_rel,
            "mean_rel": fe.mean_rel, "rms_rel": fe.rms_rel,
            "kernel_samples": [round(v, 4) for v in kern],
            "call_samples": [round(v, 4) for v in call]}


def timed_direct(eng, px, py, reps):
    eng.compute_field_direct(px, py)  # warm-up
    kern, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.compute_field_direct(px, py)
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(eng.direct_field_kernel_ms())
    return kern, call


def field_c5(reps):
    arrs = scenes.config_scene("c5")
    px, py = np.ascontiguousarray(arrs[0][:120_000]), np.ascontiguousarray(arrs[1][:120_000])
    tiled = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    tiled.reset_bodies(*arrs)
    walk = bh_amd.Engine(bh_amd.default_params(theta=0.0), device=0)
    walk.reset_bodies(*arrs)
    kern, call = timed_direct(tiled, px, py, reps)
    walk.compute_field(px, py)  # warm-up
    wkern, wcall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref = walk.compute_field(px, py)
        wcall.append((time.perf_counter() - t0) * 1e3)
        wkern.append(walk.field_kernel_ms())
    got = tiled.compute_field_direct(px, py)
    same = all(np.array_equal(g.view(np.int64), r.view(np.int64)) for g, r in zip(got, ref))
    walk.close()
    b = {"bodies": len(arrs[0]), "probes": len(px), "shape": bh_amd.direct_field_shape(len(px)),
         "direct_kernel_ms": med(kern), "direct_call_ms": med(call),
         "walk_kernel_ms": med(wkern), "walk_call_ms": med(wcall),
         "walk_over_direct": round(med(wkern) / med(kern), 3), "bit_identical": same,
         "direct_samples": [round(v, 4) for v in kern],
         "walk_samples": [round(v, 4) for v in wkern]}
    kern, call = timed_direct(tiled, px[:4096], py[:4096], reps)
    c = {"bodies": len(arrs[0]), "probes": 4096, "shape": bh_amd.direct_field_shape(4096),
         "direct_kernel_ms": med(kern), "direct_call_ms": med(call),
         "direct_samples": [round(v, 4) for v in kern], "sweep": []}
    for n in SWEEP:
        qx = np.ascontiguousarray(np.resize(arrs[0], n))
        qy = np.ascontiguousarray(np.resize(arrs[1], n))
        kern, _ = timed_direct(tiled, qx, qy, reps)
        c["sweep"].append({"probes": n, "shape": bh_amd.direct_field_shape(n),
                           "direct_kernel_ms": med(kern),
                           "ns_per_probe": round(med(kern) * 1e6 / n, 2)})
    tiled.close()
    return b, c


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"reps": reps, "warmup": 1}
    if len(sys.argv) > 2:
        out["label"] = sys.argv[2]
    out["a_c3_force_error_4096"] = force_error_c3(reps)
    out["b_c5_120000_probes"], out["c_c5_4096_probes"] = field_c5(reps)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "direct_field_timing.jsonl"), "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
