"""bh_launch_plan (host-only) and the scenes the launch-shape GPU tests are built on.

The one-GPU step picks its kernels and launch shapes from the list size.  bh_launch_plan reads
that choice out through the functions the engine itself branches on, so the sizes where it
changes are found here by bisection, never written down: a pull request that moves a threshold
moves the tests' sizes with it.  The scenes of the breadth-first walk's give-ups are checked
against tests/walk_model.py alone -- no engine, no GPU.
"""
import functools

import numpy as np

import bh_amd
import oracle
import walk_model
from bh_amd import scenes

FIELDS = bh_amd.LAUNCH_PLAN_FIELDS
# Fields that count workgroups, buckets or words: they step every few hundred bodies.  The
# others select a kernel or a wave shape.
COUNT_FIELDS = ("sort_buckets", "com_chunks", "bfs_bits", "xcd_groups", "kick_xcd_groups",
                "order_runs")
PATH_FIELDS = tuple(f for f in FIELDS if f not in COUNT_FIELDS)


@functools.lru_cache(maxsize=None)
def plan(n):
    return bh_amd.launch_plan(n)


def _changes(fields, lo, hi, out):
    """Every n in (lo, hi] where a field differs from n - 1, for fields monotone on [lo, hi]."""
    if all(plan(lo)[f] == plan(hi)[f] for f in fields):
        return
    if hi - lo == 1:
        out.add(hi)
        return
    mid = (lo + hi) // 2
    _changes(fields, lo, mid, out)
    _changes(fields, mid, hi, out)


@functools.lru_cache(maxsize=None)
def boundaries(lo, hi, fields=FIELDS):
    """Ascending list of every n in (lo, hi] whose plan differs from that of n - 1 in one of
    `fields`.  Bisection per field; a field need not be monotone over the whole range (the
    small front's width ends at 0, the remapped groups drop when the waves per workgroup step),
    only between the changes already found, so the search is repeated inside those pieces until
    nothing new turns up."""
    found = set()
    # (the kernel and wave-shape fields first: the counting fields are monotone between them)
    for f in PATH_FIELDS + tuple(f for f in fields if f not in PATH_FIELDS):
        while True:
            cuts = [lo] + sorted(found) + [hi]
            new = set()
            for a, b in zip(cuts, cuts[1:]):
                _changes((f,), a, b, new)
            if new <= found:
                break
            found |= new
    return [n for n in sorted(found) if any(plan(n)[f] != plan(n - 1)[f] for f in fields)]


def field_boundaries(field, lo, hi):
    return boundaries(lo, hi, (field,))


def ladder_sizes(lo=2, hi=70_000):
    """The sizes of the GPU ladder: b - 1 and b at every change of a kernel or wave-shape field
    in (lo, hi], at the first two and the last two changes of every counting field (one, two
    and three workgroups or words; the largest grids in range), and 2^k + 1 up to k = 12.
    The counting fields step every few hundred bodies (every 15 for the bitmap's words): all
    of their changes would be some 1 100 sizes of the same code paths."""
    cuts = set(boundaries(lo, hi, PATH_FIELDS))
    for f in COUNT_FIELDS:
        b = field_boundaries(f, lo, hi)
        cuts.update(b[:2] + b[-2:])
    sizes = {s for b in cuts for s in (b - 1, b)} | {2 ** k + 1 for k in range(1, 13)}
    return sorted(s for s in sizes if s >= lo)


# ---- the plan ---------------------------------------------------------------------------------

def test_plan_is_host_only_and_sized():
    p = plan(12_500)
    assert tuple(p) == FIELDS
    assert plan(0) == dict.fromkeys(FIELDS, 0)
    assert p["sort_buckets"] * 512 >= 12_500 and p["com_chunks"] * 1024 >= 12_500


def test_every_field_changes_below_70000():
    for f in FIELDS:
        if f in ("span_groups", "own_scan", "node_addr64"):  # their switches lie higher
            continue
        assert field_boundaries(f, 1, 70_000), f"{f} never changes for n in [1, 70 000]"


def test_high_switches_exist():
    # (node_addr64 switches once, past 10^7 bodies: tests/test_node_addressing.py)
    assert not field_boundaries("node_addr64", 1, 5_000_000)
    assert len(field_boundaries("span_groups", 70_000, 5_000_000)) >= 1
    assert len(field_boundaries("own_scan", 70_000, 5_000_000)) == 1
    assert len(field_boundaries("wpb", 70_000, 5_000_000)) == 1


def test_bodies_per_wave_never_decreases():
    for f in ("bpw", "kick_bpw"):
        prev = 0
        for b in [1] + field_boundaries(f, 1, 5_000_000):
            assert plan(b)[f] >= prev, f"{f} drops at {b}"
            prev = plan(b)[f]
        assert prev == 64


def test_small_front_width_holds_the_list():
    on = [1] + boundaries(1, 70_000, ("small_front", "small_front_p"))
    assert plan(1)["small_front"] == 1
    for n in range(1, field_boundaries("small_front", 1, 70_000)[0] + 2):  # and one by one
        p = bh_amd.launch_plan(n)
        assert p["small_front_p"] >= n if p["small_front"] else p["small_front_p"] == 0, n
    for b in on:
        for n in (b - 1, b):
            p = plan(n)
            if n >= 1 and p["small_front"]:
                P = p["small_front_p"]
                assert P >= n and P & (P - 1) == 0, f"P = {P} for {n} bodies"
                assert P < 2 * n or n == 1
            else:
                assert p["small_front_p"] == 0


def test_boundaries_equal_a_scan():
    """The bisection against a plain scan, over the range where every field of the small sizes
    switches and over one with the wave shapes' switches."""
    for lo, hi in ((1, 5_000), (65_000, 66_000)):
        want = [n for n in range(lo + 1, hi + 1) if plan(n) != plan(n - 1)]
        assert boundaries(lo, hi) == want


def test_ladder_takes_its_sizes_from_the_plan():
    sizes = ladder_sizes()
    assert 40 <= len(sizes) <= 140
    for f in PATH_FIELDS:
        for b in field_boundaries(f, 2, 70_000):
            assert b - 1 in sizes and b in sizes, f"{f} switches at {b}"
    for f in ("bpw", "kick_bpw"):  # every wave shape the plan takes in range is run
        taken = {plan(n)[f] for n in [2] + field_boundaries(f, 2, 70_000)}
        assert taken <= {plan(n)[f] for n in sizes}
        assert len(taken) >= 3


# ---- the walk model against the reference ----------------------------------------------------

def test_walk_model_counts_the_reference_visits():
    """Opened plus accepted nodes of the breadth-first model = the C oracle's visit count."""
    arrs = scenes.two_disks(1600, 1600)
    sample = np.arange(0, 3200, 7, dtype=np.int64)
    for theta in (0.5, 0.2):
        w = walk_model.walk_counts(arrs, theta=theta, bodies=sample)
        ref = oracle.Oracle(*arrs, theta=theta)
        _, _, vis = ref.accelerations(subset=sample, visits=True)
        ref.close()
        assert np.array_equal(w.visits, vis)
        assert w.nodes > 3200


# ---- the scenes of the breadth-first walk's give-ups ----------------------------------------
# Device constants (traverse.hip): BFS_E_CAP opened cells per level, BFS_A_CAP accepted nodes.
# The device also marks skip slots and jitter cells, so "below" leaves a factor 2 under the
# constant and "above" a factor 2 over it.
E_CAP, A_CAP = 128, 384


def _log_radial(n, cx, cy, r0, r1, seed):
    """n bodies at log-uniform radii: a dozen octaves of depth, a steady few cells per level."""
    rng = np.random.default_rng(seed)
    r = np.exp(rng.uniform(np.log(r0), np.log(r1), n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    return (cx + r * np.cos(phi), cy + r * np.sin(phi), np.zeros(n), np.zeros(n),
            rng.uniform(0.5, 1.5, n))


def _patch(n, x0, y0, side, seed):
    rng = np.random.default_rng(seed)
    return (x0 + side * rng.random(n), y0 + side * rng.random(n), np.zeros(n), np.zeros(n),
            rng.uniform(0.5, 1.5, n))


def _far(n, seed):
    """Bodies outside the root cell (never inserted, BHA:126): they walk a tree they see under a
    small angle."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(2500.0, 60000.0, n), rng.uniform(-20000.0, 20000.0, n), np.zeros(n),
            np.zeros(n), rng.uniform(0.5, 1.5, n))


def _pairs(n_pairs, seed, side):
    """Pairs 2e-3 apart, just above the jitter distance: every pair hangs on a chain of
    one-child cells down to the last depth.  The root is `side` wide: the deeper the tree, the
    longer the chains."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.05 * side, 0.95 * side, n_pairs)
    y = rng.uniform(0.05 * side, 0.95 * side, n_pairs)
    x = np.stack([x, x + 2e-3], axis=1).reshape(-1)
    y = np.stack([y, y], axis=1).reshape(-1)
    n = 2 * n_pairs
    return (x, y, np.zeros(n), np.zeros(n), rng.uniform(0.5, 1.5, n))


PAIR_SIDE = 1_000_000  # width_px = height_px of the pair scenes: jitter depth 29

# name -> (arrays, engine parameters)
GIVE_UP_SCENES = {
    "clean": lambda: (scenes.two_disks(1600, 1600), dict(theta=0.8)),
    "accept_overflow": lambda: (_log_radial(3000, 1200.0, 400.0, 0.05, 350.0, 1),
                                dict(theta=0.2)),
    "level_overflow": lambda: (scenes.uniform(4096, 1.0, seed=5), dict(theta=0.05)),
    "mixed": lambda: (scenes.concat(_log_radial(1200, 1900.0, 400.0, 0.05, 300.0, 1),
                                    _patch(2000, 100.0, 300.0, 400.0, 2), _far(500, 3)),
                      dict(theta=0.08)),
    "pairs_32": lambda: (_pairs(32, 11, PAIR_SIDE),
                         dict(theta=0.5, width_px=PAIR_SIDE, height_px=PAIR_SIDE)),
    "pairs_200": lambda: (_pairs(200, 12, PAIR_SIDE),
                          dict(theta=0.5, width_px=PAIR_SIDE, height_px=PAIR_SIDE)),
    "pairs_2000": lambda: (_pairs(2000, 13, PAIR_SIDE),
                           dict(theta=0.5, width_px=PAIR_SIDE, height_px=PAIR_SIDE)),
}


@functools.lru_cache(maxsize=None)
def give_up_scene(name):
    return GIVE_UP_SCENES[name]()


@functools.lru_cache(maxsize=None)
def _model(name):
    arrs, kw = give_up_scene(name)
    assert plan(len(arrs[0]))["bfs"] == 1, "the first walk of this size is not breadth first"
    return walk_model.walk_counts(arrs, **kw)


def test_scene_clean():
    w = _model("clean")
    assert w.max_opened.max() <= E_CAP // 2 and w.accepted.max() <= A_CAP // 2


def test_scene_accept_overflow():
    w = _model("accept_overflow")
    assert np.count_nonzero(w.accepted >= 2 * A_CAP) * 2 >= len(w.accepted)
    assert w.max_opened.max() < E_CAP


def test_scene_level_overflow():
    w = _model("level_overflow")
    assert np.count_nonzero(w.max_opened >= 2 * E_CAP) * 2 >= len(w.accepted)


def test_scene_mixed():
    w = _model("mixed")
    n = len(w.accepted)
    clean = (w.max_opened <= E_CAP // 2) & (w.accepted <= A_CAP // 2)
    accept = (w.accepted >= 2 * A_CAP) & (w.max_opened < E_CAP)
    level = w.max_opened >= 2 * E_CAP
    for name, cls in (("clean", clean), ("accept overflow", accept), ("level overflow", level)):
        assert np.count_nonzero(cls) * 10 >= n, f"{name}: {np.count_nonzero(cls)} of {n} bodies"
    # the level that overflows is deep, below levels that opened cells and accepted nodes
    first = np.argmax(w.opened[level] >= 2 * E_CAP, axis=1)
    assert first.min() >= 5
    assert np.all(w.opened[level][:, 1:5].min(axis=1) > 0)


def test_scene_tree_beyond_the_bitmap():
    for name in ("pairs_32", "pairs_200", "pairs_2000"):
        arrs, kw = give_up_scene(name)
        n = len(arrs[0])
        bits = plan(n)["bfs_bits"]
        assert 9 * n // 4 + 256 <= bits < 9 * n // 4 + 256 + 32
        w = _model(name)
        assert w.nodes >= 2 * (9 * n // 4 + 256), f"{name}: {w.nodes} nodes, {bits} bits"
        assert w.nodes >= 2 * bits
