#!/usr/bin/env python3
"""Potential kernel against the force kernel on the same tree state.

Usage (GPU box): python tools/potential_timing.py [reps]
C3 (theta 0.5): after one warm-up call of each, `reps` alternating pairs of a plain
compute_accelerations() (traverse_kernel_ms: the parent's k_traverse) and compute_potential()
(potential_kernel_ms), every call on a fresh build of the same state; once right after the
reset (lanes in slot order) and once after 5 steps (the Hilbert lane map live).  C5 (theta 0):
the all-pairs potential kernel beside the all-pairs force evaluation.  Prints one JSON line.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "barnes-hut-n-body_amd"))
import bh_amd  # noqa: E402
from bh_amd import scenes  # noqa: E402


def pairs(eng, reps):
    eng.set_profiling(True)
    eng.compute_accelerations()  # warm-up (and the build's jitter, once)
    eng.compute_potential()
    trav, pot = [], []
    for _ in range(reps):
        eng.compute_accelerations()
        trav.append(eng.traverse_kernel_ms()[0])
        eng.compute_potential()
        pot.append(eng.potential_kernel_ms())
    t, p = statistics.median(trav), statistics.median(pot)
    return {"traverse_kernel_ms": round(t, 4), "potential_kernel_ms": round(p, 4),
            "ratio": round(p / t, 4), "traverse_samples": [round(v, 4) for v in trav],
            "potential_samples": [round(v, 4) for v in pot]}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"reps": reps, "warmup": 1}
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c3"))
    out["c3_after_reset"] = pairs(eng, reps)
    eng.set_profiling(False)
    eng.step(5)
    out["c3_after_5_steps"] = dict(pairs(eng, reps), bodies=eng.num_bodies())
    eng.close()
    eng = bh_amd.Engine(bh_amd.default_params(theta=0.0), device=0)
    eng.reset_bodies(*scenes.config_scene("c5"))
    out["c5_all_pairs"] = dict(pairs(eng, max(1, reps // 2)), bodies=eng.num_bodies())
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
