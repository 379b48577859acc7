"""The node-address form of the tree walks (host-only): where the stock library switches from a
32-bit byte offset to a 64-bit address, and the variant library that always takes the latter.

Every kernel that walks the flattened tree exists twice (cursor_walk.hpp CursorStop::fetch); the
host picks per launch with node_off32(node_capacity) (bh_device.hpp), which bh_launch_plan reads
out as node_addr64.  The stock library switches where the node array reaches 4 GiB -- beyond any
scene a test can hold -- so the Makefile builds a second library, lib_addr64/, with the limit 0:
there every walk of every tree is the 64-bit form (tests/test_gpu_addr64.py runs them).  The
variant is only ever loaded by a fresh child process: two copies of the library never share one.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

import bh_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "barnes-hut-n-body_amd")
VARIANT = os.path.join(PKG_DIR, "lib_addr64", "libbh_engine.so")
BUILD_HINT = "make -C barnes-hut-n-body_amd -j16 ARCH=gfx950  (or __graft_entry__.build())"
NODE_BYTES = 32  # sizeof(Node), bh_device.hpp


def require_variant():
    """The variant's path; a missing library is a failure, never a skip."""
    if not os.path.isfile(VARIANT):
        pytest.fail(f"the 64-bit node-address variant {VARIANT} is not built: run {BUILD_HINT}",
                    pytrace=False)
    return VARIANT


def child_env():
    env = dict(os.environ)
    env["BH_ENGINE_LIB"] = require_variant()
    return env


def python_argv():
    """The interpreter as this process runs it (user site-packages ignored if they are here)."""
    return [sys.executable] + (["-s"] if sys.flags.no_user_site else [])


_PLAN_CHILD = """
import json, os, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bh_amd
plans = {str(n): bh_amd.launch_plan(n) for n in json.loads(sys.argv[3])}
print("PLANS " + json.dumps({"lib": os.path.realpath(bh_amd.LIB_PATH), "plans": plans}))
"""

PLAN_SIZES = (1, 2000, 4096, 100_000)


@functools.lru_cache(maxsize=None)
def variant_plans(sizes=PLAN_SIZES):
    """{n: launch_plan(n)} as the variant library answers, read by a fresh host-only child."""
    r = subprocess.run(python_argv() + ["-c", _PLAN_CHILD, ROOT, PKG_DIR, json.dumps(list(sizes))],
                       env=child_env(), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"plan child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}"
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PLANS ")][-1]
    got = json.loads(line[len("PLANS "):])
    assert got["lib"] == os.path.realpath(VARIANT), f"the child loaded {got['lib']}"
    return {int(n): p for n, p in got["plans"].items()}


def assert_variant_addresses_by_64_bits():
    """What test_gpu_addr64 asserts before it starts a child: with BH_ENGINE_LIB set as the child
    gets it, the walks of small trees take the 64-bit form and none is breadth first."""
    for n, p in variant_plans().items():
        assert p["node_addr64"] == 1 and p["bfs"] == 0, f"variant library, {n} bodies: {p}"


# ---- the stock library -------------------------------------------------------------------------

def _addr64(n, params):
    return bh_amd.launch_plan(n, params)["node_addr64"]


def _jitter_depth(width_px, height_px):
    """J: the first depth whose cell half-width is below 1e-3 (BHA:146); the root's is half the
    longer side plus 2 (BHA:360-361)."""
    h, depth = max(width_px, height_px) / 2.0 + 2.0, 0
    while not h < 1e-3:
        h, depth = h / 2.0, depth + 1
    return depth


def _formula_says_64(n, J):
    return NODE_BYTES * (n + (J + 1) * (n // 2 + 2) + 16) >= 2 ** 32


@pytest.mark.parametrize("wh", [(2400, 800), (640, 480), (1920, 1080)], ids=lambda wh: "%dx%d" % wh)
def test_switch_over_count(wh):
    params = bh_amd.default_params(width_px=wh[0], height_px=wh[1])
    lo, hi = 1, 2 ** 26
    assert _addr64(lo, params) == 0 and _addr64(hi, params) == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _addr64(mid, params) else (mid, hi)
    n_star = hi
    # a step function: 0 up to n* - 1, 1 from n* on -- around n* one by one, elsewhere on a grid
    around = range(n_star - 70, n_star + 71)
    grid = sorted({1, 2, 3, 2 ** 26} | {2 ** k + d for k in range(2, 26) for d in (-1, 0, 1)} |
                  {n_star * k // 64 for k in range(1, 192)})
    for n in list(around) + [n for n in grid if 1 <= n <= 2 ** 26]:
        assert _addr64(n, params) == (1 if n >= n_star else 0), f"{n} bodies (n* = {n_star})"
    # the same count from the capacity formula, written out independently
    J = _jitter_depth(*wh)
    assert _formula_says_64(n_star, J) and not _formula_says_64(n_star - 1, J), (n_star, J)
    if wh == (2400, 800):
        assert J == 21 and n_star == 11_184_806
        assert 10_000_000 < n_star < 12_000_000  # C4, the largest scene under test, is 12 % below
    assert _addr64(0, params) == 0  # (n = 0: every field is 0)


def test_stock_library_takes_the_32_bit_form_at_every_tested_size():
    assert os.path.realpath(bh_amd.LIB_PATH) != os.path.realpath(VARIANT)
    for n in PLAN_SIZES + (10_000_000,):
        assert bh_amd.launch_plan(n)["node_addr64"] == 0, n
    assert bh_amd.launch_plan(2000)["bfs"] == 1


# ---- the variant library -------------------------------------------------------------------

def test_variant_library_takes_the_64_bit_form_at_every_size():
    plans = variant_plans()
    assert set(plans) == set(PLAN_SIZES)
    assert all(tuple(p) == bh_amd.LAUNCH_PLAN_FIELDS for p in plans.values())
    assert_variant_addresses_by_64_bits()
    # nothing else moves: the cursor walk's own shapes are those of the stock library
    for n, p in plans.items():
        stock = bh_amd.launch_plan(n)
        for f in ("kick_bpw", "kick_wpb", "kick_xcd_groups", "cell_depth", "sort_buckets",
                  "com_chunks", "span_groups", "own_scan", "small_front", "order_runs"):
            assert p[f] == stock[f], f"{n} bodies: {f}"


def test_a_missing_variant_library_is_a_failure(monkeypatch):
    monkeypatch.setattr(sys.modules[__name__], "VARIANT", VARIANT + ".absent")
    with pytest.raises(pytest.fail.Exception, match="make -C barnes-hut-n-body_amd"):
        require_variant()


def test_every_curated_gpu_test_exists():
    """The lists of tests/test_gpu_addr64.py name tests of other modules: collected (only) in a
    child with the variant library, as the GPU children will, every id must still be there."""
    import test_gpu_addr64 as t
    ids = [i for _, family in t.CHILDREN.values() for i in family]
    assert len(set(ids)) == len(ids)
    rc, out = t.run_child("collection", ids, 300, extra=("--collect-only",))
    assert rc == 0, out[-4000:]
    listed = set(out.splitlines())
    missing = [i for i in ids if i not in listed]
    assert not missing, f"not collected: {missing}"
    assert t.loaded_libraries(out) == [os.path.realpath(VARIANT)]
    for banned in ("test_bfs_give_ups", "test_two_disks_breadth_first_walk"):
        assert not any(banned in i for i in ids)
