"""The fast walk's mixed carry (traverse.hip walk<true>: at a stop where some lanes accept the
node and others open it, the accepting lanes' terms wait for the next block) bit for bit against
the oracle, on scenes made to nest mixed stops: two tight clumps (sigma 2) inside a sparse halo, so
that single waves straddle a steep density step.  Sizes: 4 160 bodies (the first launch shape past
the breadth-first walk: 4 bodies per wave) and 65 600 (1 025 full waves).  Each scene also with
coincident pairs and massless bodies (a whole massless cell among them), with bodies outside the
root cell, and with one body beyond 2^32, whose wave takes the IEEE walk beside the fast ones.

Every case is checked three ways: the production evaluation, the counting walk with its counters,
and three steps (the fused kick-drift and kick-only walks of the pipelined step)."""
import functools

import numpy as np
import pytest

import bh_amd
import oracle
from conftest import bits_equal

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "vx", "vy", "m")
THETAS = (0.3, 0.5, 1.0, 1.6)
SIZES = (4160, 65600)
SCENES = ("clumps", "pairs_massless", "outside", "far")
W, H = 2400.0, 800.0  # the default view; the root cell is [-2, 2402] x [-802, 1602]
CLUMPS = ((700.3, 410.7), (1650.9, 380.2))
DEAD_CELL = (703.0, 413.0, 0.75)  # centre and half side of a square whose bodies are all massless


@functools.lru_cache(maxsize=None)
def scene(name, n):
    """n bodies: 35 % in each clump, the rest a uniform halo; masses in [0.5, 1.5) (no merges)."""
    rng = np.random.default_rng(1200 + n % 1000 + 7 * SCENES.index(name))
    nc = int(0.35 * n)
    x = np.concatenate([rng.normal(CLUMPS[0][0], 2.0, nc), rng.normal(CLUMPS[1][0], 2.0, nc),
                        rng.uniform(0.0, W, n - 2 * nc)])
    y = np.concatenate([rng.normal(CLUMPS[0][1], 2.0, nc), rng.normal(CLUMPS[1][1], 2.0, nc),
                        rng.uniform(0.0, H, n - 2 * nc)])
    vx, vy = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    m = rng.uniform(0.5, 1.5, n)
    halo = np.arange(2 * nc, n)
    if name == "pairs_massless":
        # 200 coincident pairs (the build's jitter cells): clump and halo bodies, each copied onto
        # a halo body.  Massless in the reference's sense is mass <= 0 (BHA:173-202: such a child
        # adds nothing to its cell, and a cell of such bodies alone is a mass-0 record): 5 % of
        # the bodies, and every body of one square inside the first clump.
        src = rng.choice(n, 200, replace=False)
        dst = rng.choice(np.setdiff1d(halo, src), 200, replace=False)
        x[dst], y[dst] = x[src], y[src]
        m[rng.choice(n, n // 20, replace=False)] *= -1.0
        cx, cy, half = DEAD_CELL
        inside = (np.abs(x - cx) < half) & (np.abs(y - cy) < half)
        assert inside.sum() >= 8, inside.sum()
        m[inside] = -np.abs(m[inside])
    elif name == "outside":  # 100 bodies outside the root cell, on all four sides (BHA:126)
        out = rng.choice(halo, 100, replace=False)
        side = np.arange(100) % 4
        d = rng.uniform(1.0, 600.0, 100)
        x[out] = np.where(side == 0, -2.0 - d, np.where(side == 1, W + 2.0 + d, x[out]))
        y[out] = np.where(side == 2, -802.0 - d, np.where(side == 3, 1602.0 + d, y[out]))
    elif name == "far":  # |x| > 2^32: lane_fast_ok fails, this body's wave walks walk<false>
        x[halo[0]] = -(2.0 ** 33 + 12345.678)
    perm = rng.permutation(n)
    return tuple(np.ascontiguousarray(a[perm]) for a in (x, y, vx, vy, m))


@functools.lru_cache(maxsize=None)
def reference(name, n, theta):
    """The oracle's side of a case, computed once: (ax, ay, visits, contributions, state after
    three steps).  Checks on the way what the tests below assume of the oracle itself."""
    arrs = scene(name, n)
    ref = oracle.Oracle(*arrs, theta=theta)
    ax, ay, vis = ref.accelerations(visits=True)
    iters, lane_visits = ref.group_union(np.arange(n))  # (the same tree; any grouping will do)
    force_iters, contribs = ref.union_force_stats()
    ref.close()
    assert np.isfinite(ax).all() and np.isfinite(ay).all()
    assert lane_visits == int(vis.sum()), "group_union walked another tree"
    assert 0 < force_iters <= iters and 0 < contribs
    assert contribs + n <= 64 * iters
    ref = oracle.Oracle(*arrs, theta=theta)
    ref.step(3)
    state = ref.get_bodies()
    ref.close()
    assert len(state[0]) == n, "a merge: the scenes are meant to have none"
    for a in (ax, ay, vis) + state:
        a.setflags(write=False)
    return ax, ay, vis, contribs, state


def _engine(arrs, theta):
    eng = bh_amd.Engine(bh_amd.default_params(theta=theta), device=0)
    eng.reset_bodies(*arrs)
    return eng


def _assert_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}"


CASES = [(name, n, theta) for n in SIZES for name in SCENES for theta in THETAS]


def test_launch_shapes():
    """4 160 bodies walk the cursor walk with 4 bodies per wave, 65 600 in 1 025 full waves."""
    small = bh_amd.launch_plan(4160, bh_amd.default_params(theta=0.5))
    assert small["bfs"] == 0 and small["bpw"] == 4, small
    big = bh_amd.launch_plan(65600, bh_amd.default_params(theta=0.5))
    assert big["bfs"] == 0 and big["bpw"] == 64 and big["kick_bpw"] == 64, big
    assert small["kick_bpw"] == 4, small


@pytest.mark.parametrize("name,n,theta", CASES)
def test_accelerations(name, n, theta):
    rax, ray, _, _, _ = reference(name, n, theta)
    eng = _engine(scene(name, n), theta)
    ax, ay = eng.compute_accelerations()
    eng.close()
    _assert_bits(ax, rax, "ax")
    _assert_bits(ay, ray, "ay")


@pytest.mark.parametrize("name,n,theta", CASES)
def test_counting_walk(name, n, theta):
    rax, ray, rvis, rcontrib, _ = reference(name, n, theta)
    eng = _engine(scene(name, n), theta)
    ax, ay, vis = eng.compute_accelerations(visits=True)
    c = eng.traversal_counters()
    eng.close()
    print(name, n, theta, c)
    _assert_bits(ax, rax, "ax")
    _assert_bits(ay, ray, "ay")
    assert np.array_equal(vis, rvis), "node-visit counts differ"
    assert c["lane_visits"] == int(rvis.sum())
    assert c["lane_contrib"] == rcontrib
    assert c["waves"] == (n + 63) // 64
    assert 0 < c["wave_blocks"] <= c["wave_iters"]
    assert c["lane_contrib"] + n <= 64 * c["wave_blocks"]


@pytest.mark.parametrize("name,n,theta", CASES)
def test_three_steps(name, n, theta):
    want = reference(name, n, theta)[4]
    eng = _engine(scene(name, n), theta)
    eng.step(3)
    got = eng.get_bodies()
    eng.close()
    assert len(got[0]) == len(want[0])
    for k, f in enumerate(FIELDS):
        _assert_bits(got[k], want[k], f)
