"""GPU: every tree walk's 64-bit node-address form (OFF32 = false, cursor_walk.hpp
CursorStop::fetch), on the library the Makefile builds with BH_NODE_OFF32_LIMIT=0 (lib_addr64/).

The stock library takes that form from 11 184 806 bodies on (tests/test_node_addressing.py): no
scene of a test reaches it.  The variant takes it for every tree, so the suite's smallest scenes
run it.  Each test here starts one fresh child process with BH_ENGINE_LIB naming the variant --
two copies of the library never share a process -- and the child runs pytest over a curated list
of the suite's own GPU tests (and of tests/addr64_cases.py): their bodies, references and
comparisons as they stand, bit for bit and exact.  Left out are the tests that assert the
breadth-first walk is taken (plan["bfs"] == 1 in test_gpu_threshold_criterion.py,
test_bfs_give_ups in test_gpu_launch_shapes.py): it has no 64-bit form, and the variant never
takes it.

One child at a time, each under its own time limit: about ten times its wall time on an MI355X
(noted beside each list; most of it is the interpreter, torch and the HIP runtime starting up),
never under 60 s.  A child that ends by a signal, at its limit or after a GPU fault fails its
test with its last output, and every later test of the module fails at once without starting
anything.  Nothing is retried and nothing skips: a missing variant library is a failure.
"""
import json
import os
import re
import subprocess
import time

import pytest

from test_node_addressing import (ROOT, VARIANT, assert_variant_addresses_by_64_bits, child_env,
                                  python_argv)

pytestmark = pytest.mark.gpu

P = "tests/test_gpu_parity.py::"
LS = "tests/test_gpu_launch_shapes.py::"
TC = "tests/test_gpu_threshold_criterion.py::"
FB = "tests/test_gpu_fallback.py::"
PO = "tests/test_gpu_potential.py::"
SL = "tests/test_gpu_step_log.py::"
FI = "tests/test_gpu_field.py::"
FG = "tests/test_gpu_field_grid.py::"
TR = "tests/test_gpu_tracers.py::"
NB = "tests/test_gpu_neighbors.py::"
GR = "tests/test_gpu_groups.py::"
KN = "tests/test_gpu_knn.py::"
A64 = "tests/addr64_cases.py::"

# family -> (time limit in seconds, node ids); the wall times are whole children, start-up included
CHILDREN = {
    # k_traverse<false, false, KICK_DRIFT | KICK_ONLY | KICK_NONE, false> at 1, 2, 32 and 64
    # bodies per wave, 1 and 8 waves per workgroup; the counting walk beside them (_evaluate)
    "step": (75, [  # 7.5 s on an MI355X
        A64 + "test_c1_baseline_ten_steps_in_one_call",
        A64 + "test_c1_baseline_ten_one_step_calls",
        A64 + "test_golden_scene_steps[merge_127-calls0]",
        A64 + "test_golden_scene_steps[jitter_306-calls1]",
        A64 + "test_golden_scene_steps[outside_153-calls2]",
        A64 + "test_last_size_of_one_wave_per_workgroup_and_first_of_eight[1]",
        A64 + "test_last_size_of_one_wave_per_workgroup_and_first_of_eight[0]",
        LS + "test_ladder[2047]",
        P + "test_tiny_and_empty[1]",
    ]),
    # k_traverse<true, false, KICK_NONE, false> (the counting walk) and the production walk
    "accelerations": (60, [  # 5.3 s on an MI355X
        A64 + "test_two_disks_600_accelerations_and_visits",
        TC + "test_counting_walk_visits_and_counters",
        P + "test_zero_and_negative_mass",
        P + "test_massless_cells_of_negative_bodies_are_not_entered[0.5]",
    ]),
    # k_traverse<false, false, KICK_OWN_DRIFT | KICK_OWN_ONLY, false> over a rank's lane range
    # and the locally essential tree's node array
    "own_kick": (65, [  # 6.4 s on an MI355X
        P + "test_multi_rank_decomposition_in_process[2-default]",
    ]),
    # the IEEE walk of the force and of the potential, NODE_SKIP on it
    "fallback": (60, [  # 4.6 s on an MI355X
        FB + "test_far_bodies[0.5]",
        FB + "test_massless_cells_on_the_fallback",
        FB + "test_potential_far_bodies[0.5]",
        FB + "test_potential_massless_cells_on_the_fallback",
    ]),
    # k_potential's fast and IEEE forms, k_traverse_pot<false> (the step log's walk)
    "potential": (60, [  # 5.6 s on an MI355X
        PO + "test_theta_sweep[0.5]",
        PO + "test_small_sizes[65]",
        PO + "test_zero_mass_bodies",
        PO + "test_diagnostics_values[two_disks]",
        SL + "test_records_equal_the_twins_diagnostics[0.5]",
        SL + "test_goldens[merge_127.npz-calls0]",
        SL + "test_negative_mass_cells",
    ]),
    # k_field<false>, k_field_grid<false>, k_tracer_step<*, false>
    "field": (60, [  # 6.1 s on an MI355X
        FI + "test_probe_counts[63]",
        FI + "test_probe_counts[130]",
        FI + "test_coincident_probes_on_the_fast_path",
        FI + "test_slot_collision_on_the_ieee_path",
        FI + "test_massless_bodies",
        FG + "test_small_grids_against_the_checker[13-7]",
        FG + "test_small_grids_against_the_checker[64-33]",
        FG + "test_massless_bodies",
        TR + "test_tracer_counts[63]",
        TR + "test_tracer_counts[130]",
        TR + "test_ieee_path",
    ]),
    # the four neighbour walks (count, nearest, fill, the pick's shrinking radius), the group
    # link walk, k_knn<*, false>
    "radius": (65, [  # 6.4 s on an MI355X
        NB + "test_two_disks_radii_and_null_outputs[8.0]",
        NB + "test_zero_and_negative_masses",
        NB + "test_pick_returns_the_callers_body",
        GR + "test_two_disks_links_and_null_outputs[8.0]",
        GR + "test_six_bodies",
        A64 + "test_groups_of_zero_and_negative_masses",
        KN + "test_two_disks_every_k_and_radius",
        KN + "test_k_around_the_size_of_S[65]",
        KN + "test_zero_and_negative_masses",
        KN + "test_nearest_returns_the_callers_bodies",
    ]),
}

# The child: pytest over the ids, then every copy of the engine library mapped into it.
_CHILD = """
import json, os, sys
import pytest
rc = int(pytest.main(["-x", "-q", "-p", "no:cacheprovider", "--durations=0"] + sys.argv[1:]))
with open("/proc/self/maps") as f:
    libs = sorted({os.path.realpath(ln.split(None, 5)[5].strip()) for ln in f
                   if "libbh_engine" in ln})
print("ADDR64-CHILD-LIBS " + json.dumps(libs), flush=True)
sys.exit(rc)
"""

FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR",
               "hipErrorLaunchFailure", "unspecified launch failure")
_dead = []  # the family whose child died: nothing is started after it


def _tail(text, lines=40):
    return "\n".join(text.splitlines()[-lines:])


def _died(family, why, out):
    _dead.append(family)
    pytest.fail(f"the child of '{family}' {why}; nothing more is started on the GPU.  Its last "
                f"output:\n{_tail(out)}", pytrace=False)


def run_child(family, ids, limit, extra=()):
    """(return code, output) of one child; fails the test if the child died."""
    argv = python_argv() + ["-c", _CHILD] + list(extra) + list(ids)
    t0 = time.monotonic()
    try:
        r = subprocess.run(argv, env=child_env(), cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=limit)
    except subprocess.TimeoutExpired as exc:
        out = exc.stdout if isinstance(exc.stdout, str) else (exc.stdout or b"").decode("utf-8",
                                                                                         "replace")
        _died(family, f"ran into its time limit of {limit} s", out)
    wall = time.monotonic() - t0
    print(f"addr64 child '{family}': {len(ids)} tests, return code {r.returncode}, "
          f"{wall:.1f} s of {limit} s")
    if r.returncode < 0 or r.returncode in (134, 139):
        _died(family, f"ended by a signal (return code {r.returncode})", r.stdout)
    if any(w in r.stdout for w in FAULT_WORDS):
        _died(family, "reported a GPU fault", r.stdout)
    return r.returncode, r.stdout


def loaded_libraries(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("ADDR64-CHILD-LIBS ")]
    assert lines, f"the child did not report its library:\n{_tail(out)}"
    return json.loads(lines[-1][len("ADDR64-CHILD-LIBS "):])


@pytest.mark.parametrize("family", list(CHILDREN))
def test_walks_by_64_bit_addresses(family):
    if _dead:
        pytest.fail(f"not run: an earlier child died ('{_dead[0]}')", pytrace=False)
    assert_variant_addresses_by_64_bits()  # host-only: the library the child will load
    limit, ids = CHILDREN[family]
    rc, out = run_child(family, ids, limit)
    assert rc == 0, f"'{family}' on the 64-bit node-address form:\n{_tail(out, 80)}"
    assert loaded_libraries(out) == [os.path.realpath(VARIANT)]
    ends = re.findall(r"^=*\s*(\d+) passed(.*?) in [\d.]+s", out, re.M)
    assert ends and int(ends[-1][0]) == len(ids) and not re.search(
        r"skipped|deselected|xfailed|xpassed", ends[-1][1]), \
        f"'{family}': not every one of the {len(ids)} listed tests ran and passed:\n{_tail(out)}"
