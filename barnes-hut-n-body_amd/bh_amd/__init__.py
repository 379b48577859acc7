"""bh_amd — Python host binding of the MI355X Barnes–Hut engine (libbh_engine.so).

Everything here is plumbing over the C-ABI in include/bh_engine.h; the physics runs in the
HIP kernels of barnes-hut-n-body_amd/csrc.  There is no CPU fallback: if the shared
library is missing or no GPU is visible, the calls fail loudly.

Two layers:
  * `Engine` — 1:1 with the C-ABI, numpy SoA arrays in/out (used by bench.py and tests).
  * `PhysicsEngine`, `Body`, `Quad`, `Config` — a mirror of the reference's Kotlin surface
    (/root/reference/src/main/kotlin/BarnesHutAlg.kt = BHA, Config.kt = CFG) with the same
    names and call pattern NBodyPanel uses, so parity tests read like the reference's use.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

from . import scenes  # noqa: F401  (re-export)

_HERE = os.path.dirname(os.path.abspath(__file__))
# BH_ENGINE_LIB selects another in-tree build of the library (A/B timing, tools/ab.sh)
LIB_PATH = os.environ.get("BH_ENGINE_LIB") or os.path.normpath(
    os.path.join(_HERE, "..", "lib", "libbh_engine.so"))

BH_OK = 0
BH_E_INVALID = -1
BH_E_DEVICE = -2
BH_E_COMM = -3
BH_E_CAPACITY = -4
BH_E_STATE = -5

EXPORTED_SYMBOLS = (
    "bh_default_params", "bh_create", "bh_create_dist", "bh_comm_unique_id", "bh_destroy",
    "bh_last_error", "bh_set_params", "bh_get_params", "bh_reset_bodies", "bh_step",
    "bh_num_bodies", "bh_get_bodies", "bh_compute_accelerations", "bh_get_quads",
    "bh_last_timings", "bh_last_tree_nodes", "bh_traverse_kernel_ms",
    "bh_traverse_kernel_samples", "bh_set_profiling",
    "bh_synchronize", "bh_shard_range", "bh_gather_slot", "bh_traversal_stats", "bh_traversal_counters", "bh_last_removed",
    "bh_selftest_fast_math", "bh_scene_galaxy_disk", "bh_scene_kepler_disk", "bh_scene_uniform",
    "bh_nbody3d_create", "bh_nbody3d_destroy", "bh_nbody3d_last_error", "bh_nbody3d_set",
    "bh_nbody3d_step", "bh_nbody3d_accelerations", "bh_nbody3d_get", "bh_nbody3d_last_ms",
    "bh_local_group_create", "bh_local_group_destroy", "bh_create_local",
    "bh_save_state", "bh_load_state", "bh_let_stats", "bh_create_solo", "bh_comm_ranks",
    "bh_debug_inject", "bh_set_mirror", "bh_map_bodies", "bh_create_multi",
    "bh_create_multi_list", "bh_multi_world", "bh_multi_member", "bh_collective_log",
    "bh_collective_log_clear", "bh_step_begin", "bh_step_positions", "bh_step_end",
    "bh_progress", "bh_compute_potential", "bh_compute_diagnostics", "bh_potential_kernel_ms",
    "bh_nbody3d_center_of_mass", "bh_default_view", "bh_render_bodies", "bh_render_kernel_ms",
    "bh_launch_plan", "bh_render_quads", "bh_render_quads_kernel_ms",
    "bh_compute_field", "bh_field_kernel_ms",
    "bh_find_neighbors", "bh_neighbors_kernel_ms", "bh_neighbor_reach",
    "bh_find_knn", "bh_find_knn_bodies", "bh_knn_kernel_ms", "bh_knn_shape",
    "bh_find_groups", "bh_groups_kernel_ms",
    "bh_compute_radial_profile", "bh_radial_profile_kernel_ms", "bh_radial_edges",
    "bh_compute_field_direct", "bh_compute_force_error", "bh_direct_field_kernel_ms",
    "bh_direct_field_shape",
    "bh_compute_field_grid", "bh_field_grid_of_view", "bh_field_grid_kernel_ms",
    "bh_field_grid_shape",
    "bh_set_tracers", "bh_num_tracers", "bh_get_tracers", "bh_tracer_kernel_ms",
    "bh_tracer_launch_shape", "bh_render_tracers",
    "bh_set_step_log", "bh_get_step_log", "bh_get_step_log_phi", "bh_step_log_kernel_ms",
)


class BhParams(ctypes.Structure):
    """struct bh_params (include/bh_engine.h) — Config fields read by step()."""
    _fields_ = [
        ("G", ctypes.c_double),
        ("dt", ctypes.c_double),
        ("theta", ctypes.c_double),
        ("soft2", ctypes.c_double),
        ("width_px", ctypes.c_int32),
        ("height_px", ctypes.c_int32),
        ("merge_max_mass", ctypes.c_double),
        ("merge_min_dist", ctypes.c_double),
    ]


class BhDiagnostics(ctypes.Structure):
    """struct bh_diagnostics (include/bh_engine.h) — the global sums of bh_compute_diagnostics."""
    _fields_ = [
        ("n", ctypes.c_int64),
        ("mass", ctypes.c_double),
        ("mx", ctypes.c_double),
        ("my", ctypes.c_double),
        ("px", ctypes.c_double),
        ("py", ctypes.c_double),
        ("lz", ctypes.c_double),
        ("kinetic", ctypes.c_double),
        ("potential", ctypes.c_double),
    ]


class BhStepRecord(ctypes.Structure):
    """struct bh_step_record (include/bh_engine.h) -- one record of the step log."""
    _fields_ = [
        ("step", ctypes.c_int64),
        ("t", ctypes.c_double),
        ("d", BhDiagnostics),
    ]


class BhForceError(ctypes.Structure):
    """struct bh_force_error (include/bh_engine.h) -- the summary of bh_compute_force_error."""
    _fields_ = [
        ("n_sample", ctypes.c_int64),
        ("n_used", ctypes.c_int64),
        ("worst", ctypes.c_int64),
        ("max_rel", ctypes.c_double),
        ("mean_rel", ctypes.c_double),
        ("rms_rel", ctypes.c_double),
    ]


class BhGroup(ctypes.Structure):
    """struct bh_group (include/bh_engine.h) -- one group of bh_find_groups' catalogue."""
    _fields_ = [
        ("label", ctypes.c_int64),
        ("count", ctypes.c_int64),
        ("first", ctypes.c_int64),
        ("mass", ctypes.c_double),
        ("mx", ctypes.c_double),
        ("my", ctypes.c_double),
        ("px", ctypes.c_double),
        ("py", ctypes.c_double),
    ]


class BhGroupsSummary(ctypes.Structure):
    """struct bh_groups_summary (include/bh_engine.h)."""
    _fields_ = [
        ("n_bodies", ctypes.c_int64),
        ("n_in_tree", ctypes.c_int64),
        ("n_groups_all", ctypes.c_int64),
        ("n_groups", ctypes.c_int64),
        ("largest_label", ctypes.c_int64),
        ("largest_count", ctypes.c_int64),
    ]


class BhRadialBin(ctypes.Structure):
    """struct bh_radial_bin (include/bh_engine.h) -- one annulus of bh_compute_radial_profile."""
    _fields_ = [
        ("count", ctypes.c_int64),
        ("mass", ctypes.c_double),
        ("mr", ctypes.c_double),
        ("mvr", ctypes.c_double),
        ("mvt", ctypes.c_double),
        ("mvr2", ctypes.c_double),
        ("mvt2", ctypes.c_double),
        ("lz", ctypes.c_double),
    ]


class BhRadialSummary(ctypes.Structure):
    """struct bh_radial_summary (include/bh_engine.h)."""
    _fields_ = [
        ("n_bodies", ctypes.c_int64),
        ("n_selected", ctypes.c_int64),
        ("n_binned", ctypes.c_int64),
        ("n_inner", ctypes.c_int64),
        ("n_outer", ctypes.c_int64),
        ("n_nan", ctypes.c_int64),
    ]


BH_RADIAL_MAX_BINS = 4096
# bh_radial_bin as a numpy record (the same 64 bytes)
RADIAL_BIN_DTYPE = np.dtype([("count", "<i8"), ("mass", "<f8"), ("mr", "<f8"), ("mvr", "<f8"),
                             ("mvt", "<f8"), ("mvr2", "<f8"), ("mvt2", "<f8"), ("lz", "<f8")])


@dataclass(frozen=True)
class RadialSummary:
    """Engine.radial_profile(): the fields of bh_radial_summary."""
    n_bodies: int
    n_selected: int
    n_binned: int
    n_inner: int
    n_outer: int
    n_nan: int


class RadialProfile:
    """Engine.radial_profile(): the edges (n_bin + 1), the raw columns of bh_radial_bin as numpy
    arrays (`bins` is the structured array itself), the summary, and derived read-outs made on
    the host with numpy, one formula each; the means and dispersions of an empty bin are NaN
    (0 / 0), not an exception, its surface density 0."""

    def __init__(self, edges, bins, summary: RadialSummary):
        self.edges = edges
        self.bins = bins
        self.summary = summary
        for name in RADIAL_BIN_DTYPE.names:
            setattr(self, name, np.ascontiguousarray(bins[name]))

    @staticmethod
    def _over(a, b):
        with np.errstate(all="ignore"):  # (an empty bin: 0 / 0 = NaN)
            return a / b

    @property
    def surface_density(self):
        """mass / (pi * (e[k+1]**2 - e[k]**2))"""
        e = self.edges
        with np.errstate(all="ignore"):
            return self.mass / (np.pi * (e[1:] ** 2 - e[:-1] ** 2))

    @property
    def v_rot(self):
        """mvt / mass"""
        return self._over(self.mvt, self.mass)

    @property
    def v_rad(self):
        """mvr / mass"""
        return self._over(self.mvr, self.mass)

    @property
    def sigma_r(self):
        """sqrt(mvr2 / mass - v_rad**2)"""
        with np.errstate(all="ignore"):
            return np.sqrt(self._over(self.mvr2, self.mass) - self.v_rad ** 2)

    @property
    def sigma_t(self):
        """sqrt(mvt2 / mass - v_rot**2)"""
        with np.errstate(all="ignore"):
            return np.sqrt(self._over(self.mvt2, self.mass) - self.v_rot ** 2)

    @property
    def mean_r(self):
        """mr / mass"""
        return self._over(self.mr, self.mass)

    @property
    def enclosed_mass(self):
        """cumsum(mass): the mass of the selected bodies in bins 0..k"""
        return np.cumsum(self.mass)


# bh_group as a numpy record (the same 64 bytes)
GROUP_DTYPE = np.dtype([("label", "<i8"), ("count", "<i8"), ("first", "<i8"), ("mass", "<f8"),
                        ("mx", "<f8"), ("my", "<f8"), ("px", "<f8"), ("py", "<f8")])


@dataclass(frozen=True)
class GroupsSummary:
    """Engine.find_groups(): the fields of bh_groups_summary."""
    n_bodies: int
    n_in_tree: int
    n_groups_all: int
    n_groups: int
    largest_label: int
    largest_count: int


@dataclass(frozen=True)
class ForceError:
    """Engine.force_error(): the sampled bodies' tree and exact accelerations and the summary of
    |a_tree - a_exact| / |a_exact| over the samples that are finite with |a_exact| > 0."""
    idx: np.ndarray
    ax_tree: np.ndarray
    ay_tree: np.ndarray
    ax_exact: np.ndarray
    ay_exact: np.ndarray
    n_sample: int
    n_used: int
    worst: int  # position in idx of max_rel (the first on ties); -1 if n_used == 0
    max_rel: float
    mean_rel: float
    rms_rel: float


class BhView(ctypes.Structure):
    """struct bh_view (include/bh_engine.h) -- the view of bh_render_bodies."""
    _fields_ = [
        ("view_x", ctypes.c_double),
        ("view_y", ctypes.c_double),
        ("zoom", ctypes.c_double),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("heavy_mass", ctypes.c_double),
    ]


class BhFieldGrid(ctypes.Structure):
    """struct bh_field_grid (include/bh_engine.h) -- the grid of bh_compute_field_grid: point
    (c, r) is (x0 + c * dx, y0 + r * dy), one multiply and one add each."""
    _fields_ = [
        ("x0", ctypes.c_double),
        ("y0", ctypes.c_double),
        ("dx", ctypes.c_double),
        ("dy", ctypes.c_double),
        ("nx", ctypes.c_int32),
        ("ny", ctypes.c_int32),
    ]


class BhFieldGridStats(ctypes.Structure):
    """struct bh_field_grid_stats (include/bh_engine.h) -- the device-made summary of the three
    planes of bh_compute_field_grid; indices are row-major, the first on ties, -1 for none."""
    _fields_ = [
        ("n_phi", ctypes.c_int64),
        ("i_phi_min", ctypes.c_int64),
        ("phi_min", ctypes.c_double),
        ("phi_max", ctypes.c_double),
        ("n_acc", ctypes.c_int64),
        ("i_a2_max", ctypes.c_int64),
        ("a2_max", ctypes.c_double),
    ]


@dataclass(frozen=True)
class Diagnostics:
    """Engine.diagnostics(): the sums of struct bh_diagnostics plus the derived quantities.
    `potential` is 0.5 * sum m * phi, or 0.0 when it was not asked for."""
    n: int
    mass: float
    mx: float
    my: float
    px: float
    py: float
    lz: float
    kinetic: float
    potential: float

    @property
    def com(self):
        """Centre of mass (sum m x / sum m, sum m y / sum m); (0, 0) if the total mass is 0."""
        if self.mass == 0.0:
            return (0.0, 0.0)
        return (self.mx / self.mass, self.my / self.mass)

    @property
    def momentum(self):
        return (self.px, self.py)

    @property
    def energy(self) -> float:
        """Kinetic + potential energy (kinetic alone without the potential)."""
        return self.kinetic + self.potential


@dataclass(frozen=True)
class StepRecord:
    """One record of Engine.get_step_log(): the step's number since the log was enabled, the sum
    of the logged steps' dt, and the Diagnostics of the state after the step's second kick."""
    step: int
    t: float
    d: Diagnostics


class BhError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__(f"bh_engine error {rc}: {msg}")
        self.rc = rc


_lib = None
_D = ctypes.POINTER(ctypes.c_double)
_I64P = ctypes.POINTER(ctypes.c_int64)
_VP = ctypes.c_void_p


def load_library(path: str | None = None):
    """Load libbh_engine.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
    lib.bh_default_params.argtypes = [ctypes.POINTER(BhParams)]
    lib.bh_default_params.restype = None
    lib.bh_create.argtypes = [ctypes.POINTER(BhParams), ctypes.c_int, ctypes.POINTER(_VP)]
    lib.bh_create_dist.argtypes = [ctypes.POINTER(BhParams), ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_VP)]
    lib.bh_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.bh_local_group_create.argtypes = [ctypes.c_int, ctypes.POINTER(_VP)]
    lib.bh_local_group_destroy.argtypes = [_VP]
    lib.bh_local_group_destroy.restype = None
    lib.bh_create_local.argtypes = [ctypes.POINTER(BhParams), ctypes.c_int, ctypes.c_int, _VP,
                                    ctypes.POINTER(_VP)]
    lib.bh_create_solo.argtypes = [ctypes.POINTER(BhParams), ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.POINTER(_VP)]
    lib.bh_create_multi.argtypes = [ctypes.POINTER(BhParams), ctypes.c_uint32, ctypes.POINTER(_VP)]
    lib.bh_create_multi_list.argtypes = [ctypes.POINTER(BhParams), ctypes.POINTER(ctypes.c_int32),
                                         ctypes.c_int32, ctypes.POINTER(_VP)]
    lib.bh_multi_world.argtypes = [_VP]
    lib.bh_multi_member.argtypes = [_VP, ctypes.c_int]
    lib.bh_multi_member.restype = _VP
    lib.bh_collective_log.argtypes = [_VP, _I64P, ctypes.c_int64, _I64P]
    lib.bh_collective_log_clear.argtypes = [_VP]
    lib.bh_destroy.argtypes = [_VP]
    lib.bh_destroy.restype = None
    lib.bh_last_error.argtypes = [_VP]
    lib.bh_last_error.restype = ctypes.c_char_p
    lib.bh_set_params.argtypes = [_VP, ctypes.POINTER(BhParams)]
    lib.bh_get_params.argtypes = [_VP, ctypes.POINTER(BhParams)]
    lib.bh_reset_bodies.argtypes = [_VP, ctypes.c_int64, _D, _D, _D, _D, _D]
    lib.bh_step.argtypes = [_VP, ctypes.c_int32]
    lib.bh_save_state.argtypes = [_VP, ctypes.c_char_p]
    lib.bh_load_state.argtypes = [_VP, ctypes.c_char_p]
    lib.bh_num_bodies.argtypes = [_VP]
    lib.bh_num_bodies.restype = ctypes.c_int64
    lib.bh_get_bodies.argtypes = [_VP, _D, _D, _D, _D, _D, ctypes.c_int64, _I64P]
    lib.bh_set_mirror.argtypes = [_VP, ctypes.c_int]
    _DPP = ctypes.POINTER(_D)
    lib.bh_map_bodies.argtypes = [_VP, _DPP, _DPP, _DPP, _DPP, _DPP, _I64P]
    lib.bh_step_begin.argtypes = [_VP, ctypes.c_int32]
    lib.bh_step_positions.argtypes = [_VP, _DPP, _DPP, _DPP,
                                      ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)), _I64P, _I64P]
    lib.bh_step_end.argtypes = [_VP]
    lib.bh_compute_accelerations.argtypes = [_VP, _D, _D, _I64P]
    lib.bh_compute_potential.argtypes = [_VP, _D]
    lib.bh_compute_diagnostics.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(BhDiagnostics)]
    lib.bh_potential_kernel_ms.argtypes = [_VP, _D]
    lib.bh_compute_field.argtypes = [_VP, ctypes.c_int64, _D, _D, _D, _D, _D, _D]
    lib.bh_field_kernel_ms.argtypes = [_VP, _D]
    lib.bh_find_neighbors.argtypes = [_VP, ctypes.c_int64, _D, _D, ctypes.c_double, _D, _I64P,
                                      _I64P, _D, _I64P, _I64P, ctypes.c_int64, _I64P]
    lib.bh_neighbors_kernel_ms.argtypes = [_VP, _D]
    lib.bh_neighbor_reach.argtypes = [ctypes.POINTER(BhParams), ctypes.c_int32, _D]
    lib.bh_find_knn.argtypes = [_VP, ctypes.c_int64, _D, _D, ctypes.c_int32, ctypes.c_double,
                                _I64P, _D, _I64P]
    lib.bh_find_knn_bodies.argtypes = [_VP, ctypes.c_int32, ctypes.c_double, _I64P, _D, _I64P,
                                       ctypes.c_int64, _I64P]
    lib.bh_knn_kernel_ms.argtypes = [_VP, _D]
    lib.bh_knn_shape.argtypes = [ctypes.c_int64, ctypes.c_int32, _I64P]
    lib.bh_find_groups.argtypes = [_VP, ctypes.c_double, ctypes.c_int64, _I64P, ctypes.c_int64,
                                   _I64P, ctypes.c_int64, ctypes.POINTER(BhGroup),
                                   ctypes.c_int64, ctypes.POINTER(BhGroupsSummary)]
    lib.bh_groups_kernel_ms.argtypes = [_VP, _D]
    lib.bh_compute_radial_profile.argtypes = [_VP] + [ctypes.c_double] * 4 + [
        ctypes.c_int32, _D, _I64P, ctypes.c_int64, ctypes.POINTER(BhRadialBin),
        ctypes.POINTER(BhRadialSummary)]
    lib.bh_radial_profile_kernel_ms.argtypes = [_VP, _D]
    lib.bh_radial_edges.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                    ctypes.c_int, _D]
    lib.bh_compute_field_direct.argtypes = [_VP, ctypes.c_int64, _D, _D, _D, _D, _D, _D]
    lib.bh_compute_force_error.argtypes = [_VP, ctypes.c_int64, _I64P, _D, _D, _D, _D,
                                           ctypes.POINTER(BhForceError)]
    lib.bh_direct_field_kernel_ms.argtypes = [_VP, _D]
    lib.bh_direct_field_shape.argtypes = [ctypes.c_int64, _I64P]
    lib.bh_compute_field_grid.argtypes = [_VP, ctypes.POINTER(BhFieldGrid), _D, _D, _D,
                                          ctypes.POINTER(BhFieldGridStats)]
    lib.bh_field_grid_of_view.argtypes = [ctypes.POINTER(BhView), ctypes.c_int32,
                                          ctypes.POINTER(BhFieldGrid)]
    lib.bh_field_grid_kernel_ms.argtypes = [_VP, _D]
    lib.bh_field_grid_shape.argtypes = [ctypes.c_int32, ctypes.c_int32, _I64P]
    lib.bh_default_view.argtypes = [ctypes.POINTER(BhView)]
    lib.bh_default_view.restype = None
    lib.bh_render_bodies.argtypes = [_VP, ctypes.POINTER(BhView), ctypes.POINTER(ctypes.c_uint8),
                                     ctypes.POINTER(ctypes.c_uint32),
                                     ctypes.POINTER(ctypes.c_uint32)]
    lib.bh_render_kernel_ms.argtypes = [_VP, _D]
    lib.bh_set_tracers.argtypes = [_VP, ctypes.c_int64, _D, _D, _D, _D]
    lib.bh_num_tracers.argtypes = [_VP]
    lib.bh_num_tracers.restype = ctypes.c_int64
    lib.bh_get_tracers.argtypes = [_VP, _D, _D, _D, _D, ctypes.c_int64, _I64P]
    lib.bh_tracer_kernel_ms.argtypes = [_VP, _D, _I64P]
    lib.bh_tracer_launch_shape.argtypes = [ctypes.c_int64, _I64P]
    lib.bh_set_step_log.argtypes = [_VP, ctypes.c_int64]
    lib.bh_get_step_log.argtypes = [_VP, ctypes.POINTER(BhStepRecord), ctypes.c_int64, _I64P]
    lib.bh_get_step_log_phi.argtypes = [_VP, _D, ctypes.c_int64, _I64P]
    lib.bh_step_log_kernel_ms.argtypes = [_VP, _D, _I64P]
    lib.bh_render_tracers.argtypes = [_VP, ctypes.POINTER(BhView),
                                      ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_uint32)]
    lib.bh_get_quads.argtypes = [_VP, _D, _D, _D, ctypes.c_int64, _I64P]
    lib.bh_render_quads.argtypes = [_VP, ctypes.POINTER(BhView), ctypes.POINTER(ctypes.c_uint32),
                                    _I64P]
    lib.bh_render_quads_kernel_ms.argtypes = [_VP, _D]
    lib.bh_last_timings.argtypes = [_VP, _D]
    lib.bh_last_tree_nodes.argtypes = [_VP]
    lib.bh_last_tree_nodes.restype = ctypes.c_int64
    lib.bh_traverse_kernel_ms.argtypes = [_VP, _D, _I64P]
    lib.bh_traverse_kernel_samples.argtypes = [_VP, _D, ctypes.c_int64, _I64P]
    lib.bh_set_profiling.argtypes = [_VP, ctypes.c_int]
    lib.bh_synchronize.argtypes = [_VP]
    lib.bh_traversal_stats.argtypes = [_VP, _I64P, _I64P, _I64P]
    lib.bh_traversal_counters.argtypes = [_VP, _I64P]
    lib.bh_let_stats.argtypes = [_VP, _I64P]
    lib.bh_comm_ranks.argtypes = [_VP, ctypes.POINTER(ctypes.c_int32),
                                  ctypes.POINTER(ctypes.c_int32)]
    lib.bh_debug_inject.argtypes = [_VP, ctypes.c_int]
    lib.bh_progress.argtypes = [_VP, _I64P]
    lib.bh_last_removed.argtypes = [_VP, _I64P, ctypes.c_int64, _I64P]
    lib.bh_shard_range.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   _I64P, _I64P]
    lib.bh_gather_slot.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
    lib.bh_gather_slot.restype = ctypes.c_int64
    lib.bh_launch_plan.argtypes = [ctypes.POINTER(BhParams), ctypes.c_int64, _I64P,
                                   ctypes.c_int64, _I64P]
    lib.bh_selftest_fast_math.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, _I64P]
    _F = ctypes.POINTER(ctypes.c_float)
    lib.bh_nbody3d_create.argtypes = [ctypes.c_int, ctypes.POINTER(_VP)]
    lib.bh_nbody3d_destroy.argtypes = [_VP]
    lib.bh_nbody3d_destroy.restype = None
    lib.bh_nbody3d_last_error.argtypes = [_VP]
    lib.bh_nbody3d_last_error.restype = ctypes.c_char_p
    lib.bh_nbody3d_set.argtypes = [_VP, ctypes.c_int64] + [_F] * 7
    lib.bh_nbody3d_step.argtypes = [_VP, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_float]
    lib.bh_nbody3d_accelerations.argtypes = [_VP, ctypes.c_float, ctypes.c_float, _F, _F, _F]
    lib.bh_nbody3d_get.argtypes = [_VP] + [_F] * 7 + [ctypes.c_int64, _I64P]
    lib.bh_nbody3d_center_of_mass.argtypes = [_VP, _D]
    lib.bh_nbody3d_last_ms.argtypes = [_VP]
    lib.bh_nbody3d_last_ms.restype = ctypes.c_double
    lib.bh_scene_galaxy_disk.argtypes = (
        [ctypes.c_int32] + [ctypes.c_double] * 6 + [ctypes.c_int32, ctypes.c_int64]
        + [ctypes.c_double] * 9 + [_D] * 5)
    lib.bh_scene_kepler_disk.argtypes = (
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int64]
        + [ctypes.c_double] * 6 + [_D] * 5)
    lib.bh_scene_uniform.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_int64,
                                     ctypes.c_int32, ctypes.c_int32] + [_D] * 5
    if path is None:
        _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(_D) if a is not None else None


def default_params(**over) -> BhParams:
    p = BhParams()
    load_library().bh_default_params(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_view(**over) -> BhView:
    v = BhView()
    load_library().bh_default_view(ctypes.byref(v))
    for k, val in over.items():
        setattr(v, k, val)
    return v


SHARD_ROUNDS = 4  # BH_SHARD_ROUNDS (include/bh_engine.h)


def shard_range(n: int, rank: int, world: int, round: int = 0):
    """Lanes [lo, hi) (Hilbert wave order) whose forces `rank` evaluates in round `round` of a
    multi-GPU evaluation (bh_shard_range): rank r owns [(r * rounds) * sub, + rounds * sub), one
    contiguous region; the accelerations of lane q sit at gather_slot(n, world, q), where round
    k's pieces are adjacent, so round k's all-gather is in place."""
    lo = ctypes.c_int64(0)
    hi = ctypes.c_int64(0)
    rc = load_library().bh_shard_range(int(n), int(rank), int(world), int(round),
                                       ctypes.byref(lo), ctypes.byref(hi))
    if rc != BH_OK:
        raise BhError(rc, "bh_shard_range: invalid arguments")
    return lo.value, hi.value


def gather_slot(n: int, world: int, lane: int) -> int:
    """Slot of lane `lane` in the exchange buffer of a multi-GPU evaluation (bh_gather_slot)."""
    g = load_library().bh_gather_slot(int(n), int(world), int(lane))
    if g < 0:
        raise BhError(BH_E_INVALID, "bh_gather_slot: invalid arguments")
    return g


# enum BH_PLAN_* (include/bh_engine.h), in order
LAUNCH_PLAN_FIELDS = (
    "small_front", "small_front_p", "cell_depth", "sort_buckets", "com_chunks", "span_groups",
    "own_scan", "bfs", "bfs_bits", "bpw", "wpb", "xcd_groups", "kick_bpw", "kick_wpb",
    "kick_xcd_groups", "order_runs", "node_addr64",
)


def launch_plan(n: int, params: BhParams | None = None) -> dict:
    """The kernels and launch shapes the one-GPU step picks for a list of `n` bodies
    (bh_launch_plan; host-only, no device): a dict keyed by LAUNCH_PLAN_FIELDS."""
    p = params if params is not None else default_params()
    out = np.zeros(len(LAUNCH_PLAN_FIELDS), dtype=np.int64)
    got = ctypes.c_int64(0)
    rc = load_library().bh_launch_plan(ctypes.byref(p), int(n), out.ctypes.data_as(_I64P),
                                       out.size, ctypes.byref(got))
    if rc != BH_OK:
        raise BhError(rc, "bh_launch_plan: invalid arguments")
    if got.value != out.size:
        raise BhError(BH_E_INVALID, "bh_launch_plan: field list out of date")
    return {k: int(v) for k, v in zip(LAUNCH_PLAN_FIELDS, out)}


def direct_field_shape(n: int):
    """(leaf records per LDS tile, lanes per workgroup, targets per lane) of the all-pairs kernel
    behind compute_field_direct and force_error for `n` targets (bh_direct_field_shape;
    host-only, no device)."""
    out = np.zeros(3, dtype=np.int64)
    rc = load_library().bh_direct_field_shape(int(n), out.ctypes.data_as(_I64P))
    if rc != BH_OK:
        raise BhError(rc, "bh_direct_field_shape: invalid arguments")
    return int(out[0]), int(out[1]), int(out[2])


def knn_shape(n: int, k: int):
    """(lanes per wave, waves per workgroup, LDS bytes per workgroup, workgroups) of the
    k-nearest walk behind find_knn and find_knn_bodies for `n` probes and lists of `k` entries
    (bh_knn_shape; host-only, no device)."""
    out = np.zeros(4, dtype=np.int64)
    rc = load_library().bh_knn_shape(int(n), int(k), out.ctypes.data_as(_I64P))
    if rc != BH_OK:
        raise BhError(rc, "bh_knn_shape: invalid arguments")
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def tracer_launch_shape(n: int):
    """(tracers per wave, waves per workgroup, steps between re-orderings of the lane map) of
    the tracer walk for `n` tracers (bh_tracer_launch_shape; host-only, no device)."""
    out = np.zeros(3, dtype=np.int64)
    rc = load_library().bh_tracer_launch_shape(int(n), out.ctypes.data_as(_I64P))
    if rc != BH_OK:
        raise BhError(rc, "bh_tracer_launch_shape: invalid arguments")
    return int(out[0]), int(out[1]), int(out[2])


def neighbor_reach(depth: int, params: BhParams | None = None) -> float:
    """The pruning bound of find_neighbors' walk at tree depth `depth` for the root cell of
    `params` (bh_neighbor_reach; host-only, no device): every findable body under a depth-`depth`
    internal node lies within this distance of the node's centre of mass."""
    p = params if params is not None else default_params()
    out = ctypes.c_double(0.0)
    rc = load_library().bh_neighbor_reach(ctypes.byref(p), int(depth), ctypes.byref(out))
    if rc != BH_OK:
        raise BhError(rc, "bh_neighbor_reach: invalid arguments")
    return out.value


def radial_edges(r_min: float, r_max: float, n_bin: int, log: bool = False) -> np.ndarray:
    """n_bin + 1 bin edges from r_min to r_max, linear or (log=True, r_min > 0) logarithmic, end
    points exact (bh_radial_edges; host-only, no device)."""
    n_bin = int(n_bin)
    out = np.zeros(max(n_bin, 0) + 1, dtype=np.float64)
    lib = load_library()
    rc = lib.bh_radial_edges(float(r_min), float(r_max), n_bin, 1 if log else 0, _dp(out))
    if rc != BH_OK:
        raise BhError(rc, lib.bh_last_error(None).decode())
    return out


def field_grid_shape(nx: int, ny: int):
    """(tile columns, tile rows, waves per workgroup, tiles) of the kernel behind
    compute_field_grid for an nx x ny grid (bh_field_grid_shape; host-only, no device)."""
    out = np.zeros(4, dtype=np.int64)
    rc = load_library().bh_field_grid_shape(int(nx), int(ny), out.ctypes.data_as(_I64P))
    if rc != BH_OK:
        raise BhError(rc, "bh_field_grid_shape: invalid arguments")
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def field_grid_of_view(view_x=0.0, view_y=0.0, zoom=1.0, width=2400, height=800, cell_px=1,
                       heavy_mass=1000.0) -> BhFieldGrid:
    """The grid under a view: one point per cell_px x cell_px block of its pixels, at the block's
    centre (bh_field_grid_of_view; host-only, no device).  Pass its fields to
    Engine.compute_field_grid."""
    lib = load_library()
    v = BhView(float(view_x), float(view_y), float(zoom), int(width), int(height),
               float(heavy_mass))
    g = BhFieldGrid()
    rc = lib.bh_field_grid_of_view(ctypes.byref(v), int(cell_px), ctypes.byref(g))
    if rc != BH_OK:
        raise BhError(rc, lib.bh_last_error(None).decode())
    return g


class NBody3D:
    """fp32 3-D all-pairs engine with the physics of the reference's OpenGL compute shader
    (gpu/GPU.kt:101-152: GpuNBody.simulate); see include/bh_engine.h bh_nbody3d_*."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._h = _VP()
        rc = self._lib.bh_nbody3d_create(int(device), ctypes.byref(self._h))
        if rc != BH_OK:
            raise BhError(rc, "bh_nbody3d_create failed")

    def _check(self, rc, what):
        if rc != BH_OK:
            raise BhError(rc, f"{what}: {self._lib.bh_nbody3d_last_error(self._h).decode()}")

    @staticmethod
    def _f(a):
        return np.ascontiguousarray(a, dtype=np.float32)

    def set(self, x, y, z, vx, vy, vz, m):
        arrs = [self._f(a) for a in (x, y, z, vx, vy, vz, m)]
        self._keep = arrs
        ptrs = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in arrs]
        self._check(self._lib.bh_nbody3d_set(self._h, len(arrs[0]), *ptrs), "bh_nbody3d_set")
        self.n = len(arrs[0])

    def step(self, k: int = 1, dt: float = 0.005, G: float = 80.0, softening: float = 1.0):
        self._check(self._lib.bh_nbody3d_step(self._h, int(k), dt, G, softening),
                    "bh_nbody3d_step")

    def accelerations(self, G: float = 80.0, softening: float = 1.0):
        out = [np.empty(self.n, dtype=np.float32) for _ in range(3)]
        ptrs = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in out]
        self._check(self._lib.bh_nbody3d_accelerations(self._h, G, softening, *ptrs),
                    "bh_nbody3d_accelerations")
        return tuple(out)

    def get(self):
        out = [np.empty(self.n, dtype=np.float32) for _ in range(7)]
        ptrs = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in out]
        got = ctypes.c_int64(0)
        self._check(self._lib.bh_nbody3d_get(self._h, *ptrs, self.n, ctypes.byref(got)),
                    "bh_nbody3d_get")
        return tuple(out)

    def center_of_mass_sums(self):
        """(sum x m, sum y m, sum z m, sum m) in fp64, reduced on the device
        (bh_nbody3d_center_of_mass): nothing but these four values is read back."""
        out = np.zeros(4, dtype=np.float64)
        self._check(self._lib.bh_nbody3d_center_of_mass(self._h, _dp(out)),
                    "bh_nbody3d_center_of_mass")
        return tuple(float(v) for v in out)

    def center_of_mass(self):
        """GpuNBodyRenderer.computeCenterOfMass() (GPU.kt:390-411): three floats, (0, 0, 0)
        for an empty or massless set."""
        sx, sy, sz, sm = self.center_of_mass_sums()
        if sm == 0.0:
            return (0.0, 0.0, 0.0)
        return (sx / sm, sy / sm, sz / sm)

    def last_ms(self) -> float:
        return float(self._lib.bh_nbody3d_last_ms(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bh_nbody3d_destroy(self._h)
            self._h = _VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def selftest_fast_math(n: int, seed: int = 1, device: int = 0) -> int:
    """Mismatches of the traversal's exact in-range sqrt/reciprocal sequences against IEEE
    sqrt, 1/sqrt, 1/x over n generated operands (bh_selftest_fast_math); 0 expected."""
    bad = ctypes.c_int64(-1)
    rc = load_library().bh_selftest_fast_math(int(device), int(n), int(seed), ctypes.byref(bad))
    if rc != BH_OK:
        raise BhError(rc, "bh_selftest_fast_math failed")
    return bad.value


def comm_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    rc = load_library().bh_comm_unique_id(buf)
    if rc != BH_OK:
        raise BhError(rc, "bh_comm_unique_id failed")
    return buf.raw


class LocalGroup:
    """In-process rank group (bh_local_group_*): the multi-GPU decomposition with device-to-
    device copies in place of RCCL, for `world` engines driven by one thread each."""

    def __init__(self, world: int):
        self._lib = load_library()
        self._h = _VP()
        rc = self._lib.bh_local_group_create(int(world), ctypes.byref(self._h))
        if rc != BH_OK:
            raise BhError(rc, "bh_local_group_create failed")
        self.world = world

    def close(self):  # after every member engine is closed
        if self._h:
            self._lib.bh_local_group_destroy(self._h)
            self._h = _VP()


class Engine:
    """The C-ABI, one call per method.  State lives in HBM; arrays are copied in/out."""

    def __init__(self, params: BhParams | None = None, device: int = 0, rank: int = 0,
                 world: int = 1, unique_id: bytes | None = None,
                 local_group: "LocalGroup | None" = None, solo: bool = False,
                 devices=None, device_mask: int | None = None):
        self._lib = load_library()
        self._h = _VP()
        self._owned = True
        self.params = params if params is not None else default_params()
        if devices is not None:  # one handle over these devices, repeats allowed (multi.cpp)
            arr = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = self._lib.bh_create_multi_list(ctypes.byref(self.params), arr, len(devices),
                                                ctypes.byref(self._h))
            world = len(devices)
        elif device_mask is not None:  # one handle over every GPU of the mask (0: all)
            rc = self._lib.bh_create_multi(ctypes.byref(self.params), int(device_mask),
                                           ctypes.byref(self._h))
            world = None
        elif solo:  # measurement: one rank's share of a `world`-rank step, alone (bh_create_solo)
            rc = self._lib.bh_create_solo(ctypes.byref(self.params), device, rank, world,
                                          ctypes.byref(self._h))
        elif local_group is not None:
            world = local_group.world
            rc = self._lib.bh_create_local(ctypes.byref(self.params), device, rank,
                                           local_group._h, ctypes.byref(self._h))
        elif world > 1 or unique_id is not None:
            rc = self._lib.bh_create_dist(ctypes.byref(self.params), device, rank, world,
                                          unique_id, ctypes.byref(self._h))
        else:
            rc = self._lib.bh_create(ctypes.byref(self.params), device, ctypes.byref(self._h))
        if rc != BH_OK:
            raise BhError(rc, "engine creation failed (is a GPU visible?)")
        if world is None:
            world = int(self._lib.bh_multi_world(self._h))
        self.rank, self.world = rank, world

    def _check(self, rc):
        if rc != BH_OK:
            raise BhError(rc, self._lib.bh_last_error(self._h).decode())

    def _kernel_ms(self, fn) -> float:
        """One of the bh_*_kernel_ms calls that return a single value."""
        ms = ctypes.c_double(0.0)
        self._check(fn(self._h, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if self._h and self._owned:
            self._lib.bh_destroy(self._h)
        self._h = _VP()

    # ---- multi-device handle ------------------------------------------------------------
    def multi_world(self) -> int:
        """Members of a bh_create_multi handle (1 for any other engine)."""
        return int(self._lib.bh_multi_world(self._h))

    def member(self, rank: int) -> "Engine":
        """Member `rank` of a multi-device handle, for diagnostics (a non-owning view: never
        step it alone -- its peers would wait for it)."""
        h = self._lib.bh_multi_member(self._h, int(rank))
        if not h:
            raise BhError(BH_E_INVALID, f"no member {rank}")
        m = Engine.__new__(Engine)
        m._lib, m._h, m._owned = self._lib, _VP(h), False
        m.params, m.rank, m.world = self.params, rank, self.world
        m._parent = self  # keeps the handle alive
        return m

    def collective_log(self):
        """(api call, site, bytes, stream) rows of every collective this engine issued
        (bh_collective_log)."""
        need = ctypes.c_int64(0)
        rc = self._lib.bh_collective_log(self._h, None, 0, ctypes.byref(need))
        if rc not in (BH_OK, BH_E_CAPACITY):
            self._check(rc)
        out = np.zeros((need.value, 4), dtype=np.int64)
        self._check(self._lib.bh_collective_log(self._h, out.ctypes.data_as(_I64P), need.value,
                                                ctypes.byref(need)))
        return out

    def collective_log_clear(self):
        self._check(self._lib.bh_collective_log_clear(self._h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params: BhParams):
        self.params = params
        self._check(self._lib.bh_set_params(self._h, ctypes.byref(params)))

    def reset_bodies(self, x, y, vx, vy, m):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, vx, vy, m)]
        n = len(arrs[0])
        if any(len(a) != n for a in arrs):
            raise ValueError("x, y, vx, vy, m must have equal lengths")
        self._check(self._lib.bh_reset_bodies(self._h, n, *[_dp(a) for a in arrs]))

    def step(self, k: int = 1):
        self._check(self._lib.bh_step(self._h, int(k)))

    def save_state(self, path: str):
        """Checkpoint: Config fields + bodies in caller order (bh_save_state)."""
        self._check(self._lib.bh_save_state(self._h, os.fsencode(path)))

    def load_state(self, path: str):
        """Resume from a bh_save_state file (params and bodies replaced)."""
        self._check(self._lib.bh_load_state(self._h, os.fsencode(path)))
        self.params = BhParams()
        self._check(self._lib.bh_get_params(self._h, ctypes.byref(self.params)))

    def num_bodies(self) -> int:
        return int(self._lib.bh_num_bodies(self._h))

    def get_bodies(self, out=None):
        """bh_get_bodies: (x, y, vx, vy, m) in caller order; `out` = five float64 arrays of at
        least N entries to fill (a caller that reuses its buffers), else new arrays."""
        n = max(self.num_bodies(), 0)  # (-1 while a call begun by step_begin runs: refused below)
        if out is None or any(len(a) < n or a.dtype != np.float64 for a in out):
            out = [np.empty(n, dtype=np.float64) for _ in range(5)]
        got = ctypes.c_int64(0)
        self._check(self._lib.bh_get_bodies(self._h, *[_dp(a) for a in out], n, ctypes.byref(got)))
        return tuple(a[: got.value] for a in out)

    def set_mirror(self, on: bool, buffers: int = 1):
        """bh_set_mirror: every step() call writes the pinned caller-order mirror itself;
        buffers=2: two of them, so map_bodies' views stay valid until the next map_bodies."""
        if buffers not in (1, 2):
            raise ValueError("buffers is 1 or 2")
        self._check(self._lib.bh_set_mirror(self._h, buffers if on else 0))

    def map_bodies(self):
        """bh_map_bodies: read-only numpy views of the pinned mirror (x, y, vx, vy, m), valid
        until the next call that changes the bodies -- copy them to keep them."""
        ptrs = [_D() for _ in range(5)]
        n = ctypes.c_int64(0)
        self._check(self._lib.bh_map_bodies(self._h, *[ctypes.byref(p) for p in ptrs],
                                            ctypes.byref(n)))
        out = []
        for p in ptrs:
            a = np.ctypeslib.as_array(p, shape=(n.value,)) if n.value else np.empty(0)
            a.flags.writeable = False
            out.append(a)
        return tuple(out)

    def step_begin(self, k: int = 1):
        """bh_step_begin: the call runs on the engine's own thread (set_mirror(True, buffers=2))."""
        self._check(self._lib.bh_step_begin(self._h, int(k)))

    def step_positions(self):
        """bh_step_positions: (x, y, m, survivors, n_before) of the running call -- read-only
        views of the mirror buffer it writes (x, y, m final) and survivor j's index in the
        list before the call."""
        ptrs = [_D() for _ in range(3)]
        sv = ctypes.POINTER(ctypes.c_uint32)()
        n, n0 = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.bh_step_positions(self._h, *[ctypes.byref(p) for p in ptrs],
                                                ctypes.byref(sv), ctypes.byref(n), ctypes.byref(n0)))
        out = [np.ctypeslib.as_array(p, shape=(n.value,)) if n.value else np.empty(0)
               for p in ptrs]
        out.append(np.ctypeslib.as_array(sv, shape=(n.value,)) if n.value
                   else np.empty(0, dtype=np.uint32))
        for a in out:
            a.flags.writeable = False
        return (*out, n0.value)

    def step_end(self):
        """bh_step_end: joins the call begun by step_begin; raises its error."""
        self._check(self._lib.bh_step_end(self._h))

    def compute_accelerations(self, visits: bool = False):
        n = self.num_bodies()
        ax = np.empty(n, dtype=np.float64)
        ay = np.empty(n, dtype=np.float64)
        vis = np.empty(n, dtype=np.int64) if visits else None
        self._check(self._lib.bh_compute_accelerations(
            self._h, _dp(ax), _dp(ay), vis.ctypes.data_as(_I64P) if visits else None))
        return (ax, ay, vis) if visits else (ax, ay)

    def compute_potential(self):
        """bh_compute_potential: phi per body in caller order.  A build, exactly as
        compute_accelerations (the jitter may move positions).  An accepted cell that contains
        the body includes the body's own mass, as its force does; theta = 0 is the exact
        softened pair potential."""
        n = max(self.num_bodies(), 0)  # (-1 while a call begun by step_begin runs: refused below)
        phi = np.empty(n, dtype=np.float64)
        self._check(self._lib.bh_compute_potential(self._h, _dp(phi)))
        return phi

    def diagnostics(self, potential: bool = True) -> Diagnostics:
        """bh_compute_diagnostics: mass, first moments, momentum, angular momentum, kinetic and
        (potential=True: a build, as compute_potential) potential energy, summed on the device
        in a fixed order.  potential=False reads the state and changes nothing."""
        d = BhDiagnostics()
        self._check(self._lib.bh_compute_diagnostics(self._h, 1 if potential else 0,
                                                     ctypes.byref(d)))
        return Diagnostics(int(d.n), d.mass, d.mx, d.my, d.px, d.py, d.lz, d.kinetic, d.potential)

    def potential_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last potential kernel launch (bh_potential_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_potential_kernel_ms)

    def compute_field(self, px, py, pm=None, want_accel=True, want_phi=True):
        """bh_compute_field: (ax, ay, phi) at the probe points (px, py), in probe order; None
        for what was not asked (want_accel: ax and ay, want_phi: phi).  A probe is a body of
        mass pm (None: 1.0, the field per unit mass) that is not in the tree: it takes every
        non-empty leaf -- a probe on a body gets that body's full term -- and the cells the
        force walk accepts, a = F / pm, phi = -G sum m / sqrt(r2 + soft2).  A build, exactly as
        compute_potential (the jitter may move positions); the probes never enter the state."""
        px = np.ascontiguousarray(px, dtype=np.float64)
        py = np.ascontiguousarray(py, dtype=np.float64)
        n = len(px)
        if px.ndim != 1 or py.shape != px.shape:
            raise ValueError("px and py must be 1-d arrays of equal length")
        if pm is not None:
            pm = np.ascontiguousarray(pm, dtype=np.float64)
            if pm.shape != px.shape:
                raise ValueError("pm must have the length of px")
        ax = np.empty(n, dtype=np.float64) if want_accel else None
        ay = np.empty(n, dtype=np.float64) if want_accel else None
        phi = np.empty(n, dtype=np.float64) if want_phi else None
        self._check(self._lib.bh_compute_field(self._h, n, _dp(px), _dp(py), _dp(pm), _dp(ax),
                                               _dp(ay), _dp(phi)))
        return ax, ay, phi

    def field_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last field kernel launch (bh_field_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_field_kernel_ms)

    def find_neighbors(self, px, py, r, lists=False, counts=True, cap=None):
        """bh_find_neighbors: the bodies within r of the probe points (px, py); r is one radius
        or an array of one per probe.  Returns (count, nearest, d2_nearest) per probe -- nearest
        is an index into get_bodies() after the call, smallest under (d2, index), -1 and +inf if
        there is none -- and with lists=True also (offsets, indices): probe j's neighbours are
        indices[offsets[j]:offsets[j + 1]], ascending.  Found iff dx*dx + dy*dy <= r*r among the
        bodies in the tree of non-zero mass; a probe on a body finds it.  counts=False (without
        lists): count is None, and the walk may shrink each probe's radius to the best distance
        so far -- the same nearest, the call for picking one body.  A build, exactly as
        compute_field (the jitter may move positions); the probes never enter the state.  A
        list capacity (cap; None: a guess) that is too small costs one re-call."""
        px = np.ascontiguousarray(px, dtype=np.float64)
        py = np.ascontiguousarray(py, dtype=np.float64)
        n = len(px)
        if px.ndim != 1 or py.shape != px.shape:
            raise ValueError("px and py must be 1-d arrays of equal length")
        pr = None
        if np.ndim(r) != 0:
            pr = np.ascontiguousarray(r, dtype=np.float64)
            if pr.shape != px.shape:
                raise ValueError("r must be a scalar or have the length of px")
        r0 = 0.0 if pr is not None else float(r)
        count = np.empty(n, dtype=np.int64) if counts or lists else None
        nearest = np.empty(n, dtype=np.int64)
        d2 = np.empty(n, dtype=np.float64)
        i64 = lambda a: a.ctypes.data_as(_I64P) if a is not None else None  # noqa: E731
        if not lists:
            self._check(self._lib.bh_find_neighbors(self._h, n, _dp(px), _dp(py), r0, _dp(pr),
                                                    i64(count), i64(nearest), _dp(d2), None,
                                                    None, 0, None))
            return count, nearest, d2
        offsets = np.empty(n + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        cap = max(64, 8 * n) if cap is None else int(cap)
        for _ in range(2):
            indices = np.empty(max(cap, 1), dtype=np.int64)
            rc = self._lib.bh_find_neighbors(self._h, n, _dp(px), _dp(py), r0, _dp(pr),
                                             i64(count), i64(nearest), _dp(d2), i64(offsets),
                                             i64(indices), cap, ctypes.byref(total))
            if rc != BH_E_CAPACITY:
                break
            cap = total.value
        self._check(rc)
        return count, nearest, d2, offsets, indices[:total.value].copy()

    def neighbors_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last find_neighbors call's device work, first walk to
        last kernel (bh_neighbors_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_neighbors_kernel_ms)

    def find_knn(self, px, py, k, r_max=float("inf")):
        """bh_find_knn: the k nearest bodies of the probe points (px, py), no farther than r_max.
        Returns (idx[n, k], d2[n, k], found[n]): row j holds the indices into get_bodies() after
        the call and the squared distances of probe j's nearest, ascending under (d2, index);
        found[j] is the number of entries, the tail of a shorter row holds -1 and +inf.  The
        candidates are the bodies in the tree of non-zero mass with dx*dx + dy*dy <= r_max*r_max;
        a probe on a body finds it with d2 = 0.  A build, exactly as compute_field (the jitter may
        move positions); the probes never enter the state."""
        px = np.ascontiguousarray(px, dtype=np.float64)
        py = np.ascontiguousarray(py, dtype=np.float64)
        n = len(px)
        if px.ndim != 1 or py.shape != px.shape:
            raise ValueError("px and py must be 1-d arrays of equal length")
        kk = max(int(k), 0)
        idx = np.empty((n, kk), dtype=np.int64)
        d2 = np.empty((n, kk), dtype=np.float64)
        found = np.empty(n, dtype=np.int64)
        self._check(self._lib.bh_find_knn(self._h, n, _dp(px), _dp(py), int(k), float(r_max),
                                          idx.ctypes.data_as(_I64P), _dp(d2),
                                          found.ctypes.data_as(_I64P)))
        return idx, d2, found

    def find_knn_bodies(self, k, r_max=float("inf")):
        """bh_find_knn_bodies: find_knn with the bodies themselves as the probes -- row i belongs
        to body i of get_bodies() after the call and holds its k nearest *other* bodies (a
        coincident other body is found with d2 = 0).  Nothing is uploaded.  Returns
        (idx[N, k], d2[N, k], found[N])."""
        kk = max(int(k), 0)
        cap = self.num_bodies()
        rows = ctypes.c_int64(0)
        for _ in range(2):
            idx = np.empty((cap, kk), dtype=np.int64)
            d2 = np.empty((cap, kk), dtype=np.float64)
            found = np.empty(cap, dtype=np.int64)
            rc = self._lib.bh_find_knn_bodies(self._h, int(k), float(r_max),
                                              idx.ctypes.data_as(_I64P), _dp(d2),
                                              found.ctypes.data_as(_I64P), cap,
                                              ctypes.byref(rows))
            if rc != BH_E_CAPACITY:
                break
            cap = rows.value
        self._check(rc)
        n = rows.value
        return idx[:n], d2[:n], found[:n]

    def knn_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last find_knn / find_knn_bodies call's device work, seed
        kernel to last store (bh_knn_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_knn_kernel_ms)

    def find_groups(self, link, min_members=1, labels=True, members=False):
        """bh_find_groups: the friends-of-friends groups of the bodies at linking length `link`.
        Returns (summary, label, groups) and with members=True also the member array: label[i]
        is the smallest list index of body i's group, -1 for a body that is not in the tree or
        has mass 0 (None with labels=False); groups is a structured array (GROUP_DTYPE) of the
        groups with at least min_members members in ascending label -- count, first, and the
        fixed-order sums mass, mx, my, px, py; group g's members are
        member_array[g.first:g.first + g.count], ascending.  Indices are into get_bodies() after
        the call.  A build, exactly as find_neighbors (the jitter may move positions).  The
        catalogue's size is learnt from a first call that asks for the summary alone."""
        n = self.num_bodies()
        sm = BhGroupsSummary()
        rc = self._lib.bh_find_groups(self._h, float(link), int(min_members), None, 0, None, 0,
                                      None, 0, ctypes.byref(sm))
        self._check(rc)
        for _ in range(2):  # (a build's jitter may change the sizes once more)
            lab = np.empty(n, dtype=np.int64) if labels else None
            mem = np.empty(max(n, 1), dtype=np.int64) if members else None
            ncat = int(sm.n_groups)
            cat = np.zeros(max(ncat, 1), dtype=GROUP_DTYPE)
            i64 = lambda a: a.ctypes.data_as(_I64P) if a is not None else None  # noqa: E731
            rc = self._lib.bh_find_groups(self._h, float(link), int(min_members), i64(lab), n,
                                          i64(mem), n, cat.ctypes.data_as(ctypes.POINTER(BhGroup)),
                                          ncat, ctypes.byref(sm))
            if rc != BH_E_CAPACITY:
                break
        self._check(rc)
        summary = GroupsSummary(int(sm.n_bodies), int(sm.n_in_tree), int(sm.n_groups_all),
                                int(sm.n_groups), int(sm.largest_label), int(sm.largest_count))
        out = (summary, lab, cat[:summary.n_groups].copy())
        return out + (mem[:summary.n_in_tree].copy(),) if members else out

    def groups_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last find_groups call's device work, link walk to last
        catalogue kernel (bh_groups_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_groups_kernel_ms)

    def radial_profile(self, cx, cy, edges, cvx=0.0, cvy=0.0, subset=None) -> RadialProfile:
        """bh_compute_radial_profile: the bodies in the annuli edges[k] <= R < edges[k+1] about
        (cx, cy), velocities taken relative to (cvx, cvy): per bin the count and the fixed-order
        sums of m, m R, m vr, m vt, m vr^2, m vt^2 and m w.  subset: list indices (a set: a
        duplicate counts once; empty selects nothing), None for every body.  No build, no
        jitter, no state change: it reads what get_bodies() returns now."""
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        n_bin = len(e) - 1
        sub = None if subset is None else np.ascontiguousarray(subset, dtype=np.int64).reshape(-1)
        # (an empty array may have a null data pointer: the subset is told by the pointer)
        sub_arg = None if sub is None else np.concatenate([sub, np.zeros(1, dtype=np.int64)])
        bins = np.zeros(max(n_bin, 1), dtype=RADIAL_BIN_DTYPE)
        sm = BhRadialSummary()
        self._check(self._lib.bh_compute_radial_profile(
            self._h, float(cx), float(cy), float(cvx), float(cvy), n_bin, _dp(e),
            None if sub is None else sub_arg.ctypes.data_as(_I64P), 0 if sub is None else len(sub),
            bins.ctypes.data_as(ctypes.POINTER(BhRadialBin)), ctypes.byref(sm)))
        summary = RadialSummary(int(sm.n_bodies), int(sm.n_selected), int(sm.n_binned),
                                int(sm.n_inner), int(sm.n_outer), int(sm.n_nan))
        return RadialProfile(e, bins[:max(n_bin, 0)], summary)

    def radial_profile_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last radial_profile call's device work, staging to last
        emit kernel (bh_radial_profile_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_radial_profile_kernel_ms)

    def compute_field_direct(self, px, py, pm=None, want_accel=True, want_phi=True):
        """bh_compute_field_direct: compute_field with no cell ever accepted, whatever the
        engine's theta -- every non-empty leaf is summed, by a tiled all-pairs kernel.  Same
        arguments, results and state semantics; bit-identical to compute_field on an engine
        that holds the same state with theta = 0."""
        px = np.ascontiguousarray(px, dtype=np.float64)
        py = np.ascontiguousarray(py, dtype=np.float64)
        n = len(px)
        if px.ndim != 1 or py.shape != px.shape:
            raise ValueError("px and py must be 1-d arrays of equal length")
        if pm is not None:
            pm = np.ascontiguousarray(pm, dtype=np.float64)
            if pm.shape != px.shape:
                raise ValueError("pm must have the length of px")
        ax = np.empty(n, dtype=np.float64) if want_accel else None
        ay = np.empty(n, dtype=np.float64) if want_accel else None
        phi = np.empty(n, dtype=np.float64) if want_phi else None
        self._check(self._lib.bh_compute_field_direct(self._h, n, _dp(px), _dp(py), _dp(pm),
                                                      _dp(ax), _dp(ay), _dp(phi)))
        return ax, ay, phi

    def force_error(self, idx=None, sample=4096, seed=0) -> ForceError:
        """bh_compute_force_error: the tree's accelerations of sampled bodies at the engine's
        theta beside their exact (theta = 0) ones, from one build, and the summary of the
        relative error.  idx: indices into the list get_bodies() returns (any order, duplicates
        allowed); None draws min(sample, N) distinct ones with np.random.default_rng(seed),
        sorted.  State semantics of compute_accelerations."""
        if idx is None:
            n = max(self.num_bodies(), 0)
            idx = np.sort(np.random.default_rng(seed).choice(n, min(int(sample), n),
                                                             replace=False))
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.ndim != 1:
            raise ValueError("idx must be a 1-d array")
        k = len(idx)
        out = [np.empty(k, dtype=np.float64) for _ in range(4)]
        s = BhForceError()
        self._check(self._lib.bh_compute_force_error(
            self._h, k, idx.ctypes.data_as(_I64P), *[_dp(a) for a in out], ctypes.byref(s)))
        return ForceError(idx, *out, int(s.n_sample), int(s.n_used), int(s.worst), s.max_rel,
                          s.mean_rel, s.rms_rel)

    def direct_field_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last all-pairs kernel launch of compute_field_direct or
        force_error (bh_direct_field_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_direct_field_kernel_ms)

    def compute_field_grid(self, x0, y0, dx, dy, nx, ny, want_accel=True, want_phi=True,
                           want_stats=False):
        """bh_compute_field_grid: (ax, ay, phi) on the regular grid whose point (c, r) is
        (x0 + c * dx, y0 + r * dy), as arrays of shape (ny, nx); None for what was not asked
        (want_accel: ax and ay, want_phi: phi).  Each value is, bit for bit, what compute_field
        returns for that coordinate with pm = None; the points are made on the device, nothing
        is uploaded or sorted.  want_stats: a fourth result, the BhFieldGridStats the device
        reduces from the three planes -- with want_accel = want_phi = False nothing else comes
        back.  A build, exactly as compute_field."""
        g = BhFieldGrid(float(x0), float(y0), float(dx), float(dy), int(nx), int(ny))
        ok = 1 <= g.nx <= 16384 and 1 <= g.ny <= 16384  # (else refused below: no planes)
        shape = (g.ny, g.nx) if ok else (1, 1)
        ax = np.empty(shape, dtype=np.float64) if want_accel else None
        ay = np.empty(shape, dtype=np.float64) if want_accel else None
        phi = np.empty(shape, dtype=np.float64) if want_phi else None
        stats = BhFieldGridStats() if want_stats else None
        self._check(self._lib.bh_compute_field_grid(
            self._h, ctypes.byref(g), _dp(ax), _dp(ay), _dp(phi),
            ctypes.byref(stats) if want_stats else None))
        return (ax, ay, phi, stats) if want_stats else (ax, ay, phi)

    def field_grid_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last grid field kernel launch (bh_field_grid_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_field_grid_kernel_ms)

    def render_bodies(self, view_x=0.0, view_y=0.0, zoom=1.0, width=None, height=None,
                      heavy_mass=1000.0, owner=False, counts=False, pixels=True, out=None):
        """bh_render_bodies: NBodyPanel.paintComponent's body pass (PNL:302-307) over the list
        get_bodies() would return, rasterised on the device.  Returns `pixels`, uint8 of shape
        (height, width): 0 nothing, 1 white, 2 black (m >= heavy_mass); with owner= / counts=
        the tuple (pixels, owner, counts), None for planes not asked for -- owner: uint32, the
        list index that painted last (0xFFFFFFFF: none), counts: uint32 bodies per pixel.
        width and height default to the engine's width_px and height_px.  out: a (pixels,
        owner, counts) tuple of C-contiguous arrays of that shape and dtype to fill instead of
        new ones (None for a plane not asked for).  Reads the state and changes nothing."""
        v = BhView(float(view_x), float(view_y), float(zoom),
                   int(self.params.width_px if width is None else width),
                   int(self.params.height_px if height is None else height), float(heavy_mass))
        ok = 1 <= v.width <= 16384 and 1 <= v.height <= 16384  # (else refused below: no planes)
        shape = (v.height, v.width) if ok else (1, 1)
        def plane(asked, k, dtype):
            if not asked:
                return None
            a = out[k] if out is not None else None
            if a is None:
                return np.empty(shape, dtype=dtype)
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError(f"out[{k}] must be a C-contiguous {np.dtype(dtype)} array of "
                                 f"shape {shape}")
            return a

        pix = plane(pixels, 0, np.uint8)
        own = plane(owner, 1, np.uint32)
        cnt = plane(counts, 2, np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(self._lib.bh_render_bodies(
            self._h, ctypes.byref(v),
            pix.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if pixels else None,
            own.ctypes.data_as(u32p) if owner else None,
            cnt.ctypes.data_as(u32p) if counts else None))
        return (pix, own, cnt) if (owner or counts or not pixels) else pix

    def render_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last render_bodies' two kernels (bh_render_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_render_kernel_ms)

    def set_tracers(self, x, y, vx=None, vy=None):
        """bh_set_tracers: replace the engine's tracer list -- massless test particles of mass
        1.0 that every step() walks over the bodies' own trees and integrates with the same
        leapfrog, and that exert nothing.  vx, vy None: zeros; empty x, y: no tracers.  One-GPU
        engines only (BH_E_STATE otherwise, unless the list is empty)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if x.ndim != 1 or y.shape != x.shape:
            raise ValueError("x and y must be 1-d arrays of equal length")
        v = []
        for a in (vx, vy):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != x.shape:
                    raise ValueError("vx and vy must have the length of x")
            v.append(a)
        self._check(self._lib.bh_set_tracers(self._h, len(x), _dp(x), _dp(y), _dp(v[0]),
                                             _dp(v[1])))

    def num_tracers(self) -> int:
        return int(self._lib.bh_num_tracers(self._h))

    def get_tracers(self):
        """bh_get_tracers: (x, y, vx, vy) of the tracers, in list order."""
        n = max(self.num_tracers(), 0)
        out = [np.empty(n, dtype=np.float64) for _ in range(4)]
        got = ctypes.c_int64(0)
        self._check(self._lib.bh_get_tracers(self._h, *[_dp(a) for a in out], n,
                                             ctypes.byref(got)))
        return tuple(out)

    def tracer_kernel_ms(self):
        """(average HIP-event ms, launches) of the tracer walks of the last step() call
        (bh_tracer_kernel_ms); (0.0, 0) unless set_profiling(True)."""
        ms = ctypes.c_double(0.0)
        k = ctypes.c_int64(0)
        self._check(self._lib.bh_tracer_kernel_ms(self._h, ctypes.byref(ms), ctypes.byref(k)))
        return ms.value, k.value

    def set_step_log(self, capacity: int):
        """bh_set_step_log: a ring of `capacity` records (1..2**20) that every step of every
        step() call appends its conservation read-out to, on the device and without a host wait;
        the ring starts empty with step and t at 0.  0: off, buffers freed.  One-GPU engines only
        (BH_E_STATE otherwise, unless capacity is 0)."""
        self._check(self._lib.bh_set_step_log(self._h, int(capacity)))

    def get_step_log(self):
        """bh_get_step_log: the logged records, oldest first, as a list of StepRecord(step, t, d)
        -- d the Diagnostics of the state after the step's second kick and before its merge rule,
        the potential from the step's own second traversal."""
        n = ctypes.c_int64(0)
        rc = self._lib.bh_get_step_log(self._h, None, 0, ctypes.byref(n))
        if rc not in (0, -4):  # (BH_E_CAPACITY: the count)
            self._check(rc)
        recs = (BhStepRecord * max(n.value, 1))()
        self._check(self._lib.bh_get_step_log(self._h, recs, n.value, ctypes.byref(n)))
        return [StepRecord(int(r.step), r.t,
                           Diagnostics(int(r.d.n), r.d.mass, r.d.mx, r.d.my, r.d.px, r.d.py, r.d.lz,
                                       r.d.kinetic, r.d.potential))
                for r in recs[:n.value]]

    def get_step_log_phi(self):
        """bh_get_step_log_phi: phi of every body of the last logged step, in the order of that
        step's list (before its merge rule).  BH_E_STATE if no step was logged since the log was
        enabled or the bodies were replaced."""
        n = ctypes.c_int64(0)
        rc = self._lib.bh_get_step_log_phi(self._h, None, 0, ctypes.byref(n))
        if rc not in (0, -4):
            self._check(rc)
        phi = np.empty(max(n.value, 0), dtype=np.float64)
        self._check(self._lib.bh_get_step_log_phi(self._h, _dp(phi), len(phi), ctypes.byref(n)))
        return phi

    def step_log_kernel_ms(self):
        """(average HIP-event ms per step, steps) of the log's staging and reduction in the last
        step() call (bh_step_log_kernel_ms); (0.0, 0) unless set_profiling(True)."""
        ms = ctypes.c_double(0.0)
        k = ctypes.c_int64(0)
        self._check(self._lib.bh_step_log_kernel_ms(self._h, ctypes.byref(ms), ctypes.byref(k)))
        return ms.value, k.value

    def render_tracers(self, view_x=0.0, view_y=0.0, zoom=1.0, width=None, height=None,
                       owner=True, counts=True):
        """bh_render_tracers: the tracer pass of a frame with render_bodies' pixel rule.
        Returns (owner, counts), uint32 of shape (height, width), None for a plane not asked
        for: the largest tracer index drawn on each pixel (0xFFFFFFFF: none) and the number of
        tracers drawn on it.  Reads the tracers and changes nothing."""
        v = BhView(float(view_x), float(view_y), float(zoom),
                   int(self.params.width_px if width is None else width),
                   int(self.params.height_px if height is None else height), 1000.0)
        ok = 1 <= v.width <= 16384 and 1 <= v.height <= 16384  # (else refused below: no planes)
        shape = (v.height, v.width) if ok else (1, 1)
        own = np.empty(shape, dtype=np.uint32) if owner else None
        cnt = np.empty(shape, dtype=np.uint32) if counts else None
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(self._lib.bh_render_tracers(
            self._h, ctypes.byref(v), own.ctypes.data_as(u32p) if owner else None,
            cnt.ctypes.data_as(u32p) if counts else None))
        return own, cnt

    def last_removed(self):
        """Indices (list before the last step() call) removed by the merge rule, ascending."""
        need = ctypes.c_int64(0)
        rc = self._lib.bh_last_removed(self._h, None, 0, ctypes.byref(need))
        if rc not in (BH_OK, BH_E_CAPACITY):
            self._check(rc)
        out = np.empty(need.value, dtype=np.int64)
        self._check(self._lib.bh_last_removed(self._h, out.ctypes.data_as(_I64P), need.value,
                                              ctypes.byref(need)))
        return out

    def get_quads(self):
        need = ctypes.c_int64(0)
        rc = self._lib.bh_get_quads(self._h, None, None, None, 0, ctypes.byref(need))
        if rc not in (BH_OK, BH_E_CAPACITY):
            self._check(rc)
        n = need.value
        cx, cy, h = (np.empty(n, dtype=np.float64) for _ in range(3))
        self._check(self._lib.bh_get_quads(self._h, _dp(cx), _dp(cy), _dp(h), n, ctypes.byref(need)))
        return cx, cy, h

    def render_quads(self, view_x=0.0, view_y=0.0, zoom=1.0, width=None, height=None,
                     heavy_mass=1000.0, lines=True, out=None):
        """bh_render_quads: NBodyPanel.paintComponent's quadtree overlay (PNL:326-344) over the
        cells get_quads() would return, rasterised on the device.  Returns (lines, n_quads):
        `lines`, uint32 of shape (height, width), counts the line draws that cover each pixel (a
        cell's corner counts 2); n_quads is len(get_quads()[0]).  lines=None (or False): the count
        only, (None, n_quads), and no image work.  width and height default to the engine's
        width_px and height_px.  out: a C-contiguous uint32 array of that shape to fill instead
        of a new one.  State semantics are get_quads()': a dropped tree cache is rebuilt, and
        that build's jitter moves bodies."""
        v = BhView(float(view_x), float(view_y), float(zoom),
                   int(self.params.width_px if width is None else width),
                   int(self.params.height_px if height is None else height), float(heavy_mass))
        want = lines is not None and lines is not False
        ok = 1 <= v.width <= 16384 and 1 <= v.height <= 16384  # (else refused below: no plane)
        shape = (v.height, v.width) if ok else (1, 1)
        img = None
        if want:
            img = out if out is not None else np.empty(shape, dtype=np.uint32)
            if img.shape != shape or img.dtype != np.uint32 or not img.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous uint32 array of shape {shape}")
        n = ctypes.c_int64(0)
        self._check(self._lib.bh_render_quads(
            self._h, ctypes.byref(v),
            img.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if want else None,
            ctypes.byref(n)))
        return img, int(n.value)

    def render_quads_kernel_ms(self) -> float:
        """HIP-event time (ms) of the last render_quads' kernels (bh_render_quads_kernel_ms)."""
        return self._kernel_ms(self._lib.bh_render_quads_kernel_ms)

    def let_stats(self):
        """Multi-rank build sharding: LET builds, full builds, last subset size, last LET nodes."""
        out = np.zeros(5, dtype=np.int64)
        self._check(self._lib.bh_let_stats(self._h, out.ctypes.data_as(_I64P)))
        d = dict(zip(("let_builds", "full_builds", "subset", "let_nodes", "overflows"),
                     out.tolist()))
        return d

    def comm_ranks(self):
        """(ncclCommCount, ncclCommUserRank) of the engine's RCCL communicator; (0, rank) for
        an engine without one (bh_comm_ranks)."""
        c, r = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.bh_comm_ranks(self._h, ctypes.byref(c), ctypes.byref(r)))
        return c.value, r.value

    def debug_inject(self, what: int = 1):
        """Test hook (bh_debug_inject): 1 = the next LET build of this rank trips its guard;
        2 + k = the k-th next full build raises its jitter flag; 100 + k / 200 + k = this rank
        fails host-side before its k-th next collective / group barrier."""
        self._check(self._lib.bh_debug_inject(self._h, int(what)))

    def progress(self):
        """bh_progress (any thread, also while a call runs): dict of api_calls, collectives,
        last_site, busy, failed, comm_aborted."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._lib.bh_progress(self._h, out.ctypes.data_as(_I64P)))
        f = int(out[3])
        return {"api_calls": int(out[0]), "collectives": int(out[1]), "last_site": int(out[2]),
                "busy": bool(f & 1), "failed": bool(f & 2), "comm_aborted": bool(f & 4)}

    def set_profiling(self, on: bool):
        self._check(self._lib.bh_set_profiling(self._h, 1 if on else 0))

    def last_timings(self):
        out = np.zeros(5, dtype=np.float64)
        self._check(self._lib.bh_last_timings(self._h, _dp(out)))
        return dict(zip(("build", "traverse", "integrate", "merge", "allgather"), out.tolist()))

    def traverse_kernel_ms(self):
        avg = ctypes.c_double(0.0)
        cnt = ctypes.c_int64(0)
        self._check(self._lib.bh_traverse_kernel_ms(self._h, ctypes.byref(avg), ctypes.byref(cnt)))
        return avg.value, cnt.value

    def traverse_kernel_samples(self):
        """Per-launch traversal kernel times (ms) of the last step() call, in launch order."""
        need = ctypes.c_int64(0)
        rc = self._lib.bh_traverse_kernel_samples(self._h, None, 0, ctypes.byref(need))
        if rc not in (BH_OK, BH_E_CAPACITY):
            self._check(rc)
        out = np.empty(need.value, dtype=np.float64)
        self._check(self._lib.bh_traverse_kernel_samples(self._h, _dp(out), need.value,
                                                         ctypes.byref(need)))
        return out

    def traversal_stats(self):
        """(lane visits, wave iterations, waves) of the last compute_accelerations(visits=True);
        lane efficiency = lane_visits / (64 * wave_iters)."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.bh_traversal_stats(self._h, ctypes.byref(a), ctypes.byref(b),
                                                 ctypes.byref(c)))
        return a.value, b.value, c.value

    def traversal_counters(self):
        """Counters of the last compute_accelerations(visits=True) (bh_traversal_counters):
        dict of lane_visits, lane_contrib, wave_iters, wave_blocks, waves."""
        out = np.zeros(5, dtype=np.int64)
        self._check(self._lib.bh_traversal_counters(self._h, out.ctypes.data_as(_I64P)))
        return dict(zip(("lane_visits", "lane_contrib", "wave_iters", "wave_blocks", "waves"),
                        (int(v) for v in out)))

    def last_tree_nodes(self) -> int:
        return int(self._lib.bh_last_tree_nodes(self._h))

    def synchronize(self):
        self._check(self._lib.bh_synchronize(self._h))


# ---- mirror of the reference's Kotlin surface ----------------------------------------------

@dataclass
class Body:  # BHA:21-25
    x: float
    y: float
    vx: float
    vy: float
    m: float


@dataclass(frozen=True)
class Quad:  # BHA:53-82
    cx: float
    cy: float
    h: float

    def contains(self, b: Body) -> bool:  # BHA:61-62
        return (b.x >= self.cx - self.h and b.x < self.cx + self.h
                and b.y >= self.cy - self.h and b.y < self.cy + self.h)

    def child(self, which: int) -> "Quad":  # BHA:73-81
        hh = self.h / 2.0
        return Quad(self.cx + (hh if which & 1 else -hh), self.cy + (hh if which & 2 else -hh), hh)


class Config:  # CFG:2-39 — mutable globals read live by step()
    WIDTH_PX = 2400
    HEIGHT_PX = 800
    G = 80.0
    DT = 0.005
    SOFTENING = 1.0
    SOFT2 = 1.0 * 1.0
    theta = 0.30
    R = 100.0
    N = 5000
    CENTRAL_MASS = 50_000.0
    MIN_R = 8.0
    TOTAL_SATELLITE_MASS = 5_000.0


class BHTree:
    """getTreeForDebug() result: visitQuads (BHA:265-274) over a pre-order quad list."""

    def __init__(self, cx, cy, h):
        self._q = (cx, cy, h)

    def visit_quads(self, visit):
        cx, cy, h = self._q
        for i in range(len(cx)):
            visit(Quad(float(cx[i]), float(cy[i]), float(h[i])))

    visitQuads = visit_quads


class PhysicsEngine:
    """PhysicsEngine(initialBodies) (BHA:287) — writes results back into the same Body
    objects (BHA:414-432) and shrinks the caller's list on a merge (BHA:519)."""

    def __init__(self, initial_bodies: list, device: int = 0, devices=None):
        self._bodies = initial_bodies
        self.merge_max_mass = 4_000.0          # BHA:315
        self.merge_min_dist = Config.MIN_R     # BHA:321
        # devices: one handle over several GPUs (bh_create_multi_list), else one GPU
        self._eng = Engine(self._params(), device=device, devices=devices)
        self._push()

    def _params(self) -> BhParams:
        return default_params(G=Config.G, dt=Config.DT, theta=Config.theta, soft2=Config.SOFT2,
                              width_px=int(Config.WIDTH_PX), height_px=int(Config.HEIGHT_PX),
                              merge_max_mass=self.merge_max_mass,
                              merge_min_dist=self.merge_min_dist)

    def _soa(self):
        bs = self._bodies
        return np.array([[b.x, b.y, b.vx, b.vy, b.m] for b in bs], dtype=np.float64).reshape(-1, 5)

    def _push(self):
        soa = self._soa()
        self._eng.reset_bodies(*soa.T)
        self._shadow = soa

    def _changed(self) -> bool:
        """Whether the caller's bodies differ (bitwise) from what the engine holds; step()
        re-uploads only then, so the engine keeps its Morton-ordered state across frames."""
        soa = self._soa()
        return soa.shape != self._shadow.shape or not np.array_equal(
            soa.view(np.int64), self._shadow.view(np.int64))

    def _pull(self, after_step=False):
        x, y, vx, vy, m = self._eng.get_bodies()
        n = len(x)
        bs = self._bodies
        if after_step:
            rem = self._eng.last_removed()  # BHA:519 removeAt on the caller's list ...
            if len(rem) <= 2:
                for j in rem[::-1]:
                    del bs[int(j)]
            elif len(rem):  # ... as one pass: the same survivors, objects and list kept
                gone = set(int(j) for j in rem)
                bs[:] = [b for i, b in enumerate(bs) if i not in gone]
        if len(bs) != n:
            raise RuntimeError("engine and caller body lists diverged")
        for i in range(n):
            b = bs[i]
            b.x, b.y, b.vx, b.vy, b.m = float(x[i]), float(y[i]), float(vx[i]), float(vy[i]), float(m[i])
        self._shadow = np.stack([x, y, vx, vy, m], axis=1) if n else np.zeros((0, 5))

    def step(self):  # BHA:405-439
        self._eng.set_params(self._params())
        if self._changed():  # the caller edited bodies between frames
            self._push()
        self._eng.step(1)
        self._pull(after_step=True)

    def get_bodies(self):  # BHA:335
        return self._bodies

    def reset_bodies(self, new_bodies: list):  # BHA:342-349
        self._bodies = new_bodies
        self._push()

    def get_tree_for_debug(self) -> BHTree:  # BHA:329-332
        self._eng.set_params(self._params())
        cx, cy, h = self._eng.get_quads()
        self._pull()
        return BHTree(cx, cy, h)

    def diagnostics(self, potential: bool = True) -> Diagnostics:
        """Conservation read-out of the caller's list (Engine.diagnostics; the reference has
        none).  potential=True builds a tree as step()'s first half does, so its jitter is
        written back into the Body objects."""
        self._eng.set_params(self._params())
        if self._changed():
            self._push()
        d = self._eng.diagnostics(potential)
        if potential:
            self._pull()
        return d

    def render(self, view_x=0.0, view_y=0.0, zoom=1.0, width=None, height=None,
               heavy_mass=1000.0, owner=False, counts=False):
        """NBodyPanel.paintComponent's body pass over the caller's list (Engine.render_bodies).
        Nothing is pulled back: the call changes nothing."""
        self._eng.set_params(self._params())
        if self._changed():
            self._push()
        return self._eng.render_bodies(view_x, view_y, zoom, width, height, heavy_mass,
                                       owner=owner, counts=counts)

    def render_tree(self, view_x=0.0, view_y=0.0, zoom=1.0, width=None, height=None):
        """NBodyPanel.paintComponent's quadtree overlay of getTreeForDebug()'s tree
        (Engine.render_quads): (lines, n_quads).  As get_tree_for_debug, a fresh tree's jitter
        is written back into the Body objects."""
        self._eng.set_params(self._params())
        got = self._eng.render_quads(view_x, view_y, zoom, width, height)
        self._pull()
        return got

    def pick(self, x, y, r):
        """The Body of the caller's list nearest to (x, y) within r -- the body under the cursor
        -- or None (Engine.find_neighbors: among the bodies in the tree of non-zero mass, ties to
        the lower list index).  Builds a tree as step()'s first half does, so its jitter is
        written back into the Body objects."""
        self._eng.set_params(self._params())
        if self._changed():
            self._push()
        _, nearest, _ = self._eng.find_neighbors([float(x)], [float(y)], float(r), counts=False)
        self._pull()
        return self._bodies[int(nearest[0])] if nearest[0] >= 0 else None

    def nearest(self, x, y, k, r_max=float("inf")):
        """The up to k Body objects of the caller's list nearest to (x, y) and no farther than
        r_max, nearest first, ties to the lower list index (Engine.find_knn: among the bodies in
        the tree of non-zero mass).  Builds a tree as step()'s first half does, so its jitter is
        written back into the Body objects."""
        self._eng.set_params(self._params())
        if self._changed():
            self._push()
        idx, _, found = self._eng.find_knn([float(x)], [float(y)], int(k), float(r_max))
        self._pull()
        return [self._bodies[int(c)] for c in idx[0, :int(found[0])]]

    def groups(self, link, min_members=2):
        """The friends-of-friends groups of the caller's list at linking length `link`
        (Engine.find_groups): a list of lists of the caller's own Body objects, one per group of
        at least min_members members, in catalogue order (ascending lowest list index; within a
        group ascending list index).  Builds a tree as step()'s first half does, so its jitter is
        written back into the Body objects; bodies outside the root cell or of mass 0 are in no
        group."""
        self._eng.set_params(self._params())
        if self._changed():
            self._push()
        _, _, cat, mem = self._eng.find_groups(float(link), int(min_members), labels=False,
                                               members=True)
        self._pull()
        bs = self._bodies
        return [[bs[int(c)] for c in mem[int(g["first"]):int(g["first"] + g["count"])]]
                for g in cat]

    def profile(self, x, y, edges, vx=0.0, vy=0.0, bodies=None) -> RadialProfile:
        """The radial profile of the caller's list about (x, y) in the frame moving with
        (vx, vy) (Engine.radial_profile).  bodies: the caller's own Body objects to select, told
        by identity -- one list of groups(), for instance -- else every body.  Nothing is pulled
        back: the call changes nothing."""
        self._eng.set_params(self._params())
        if self._changed():
            self._push()
        subset = None
        if bodies is not None:
            at = {id(b): i for i, b in enumerate(self._bodies)}
            try:
                subset = [at[id(b)] for b in bodies]
            except KeyError:
                raise ValueError("profile: a body of `bodies` is not in the engine's list") from None
        return self._eng.radial_profile(float(x), float(y), edges, float(vx), float(vy), subset)

    getBodies = get_bodies
    resetBodies = reset_bodies
    getTreeForDebug = get_tree_for_debug

    @property
    def engine(self) -> Engine:
        return self._eng
