/*
 * bh_engine.h — C-ABI drop-in boundary of the MI355X Barnes–Hut engine.
 *
 * Replaces the reference's PhysicsEngine / Body / BHTree Kotlin surface
 * (/root/reference/src/main/kotlin/BarnesHutAlg.kt = BHA, Config.kt = CFG) as consumed by
 * NBodyPanel (NBodyPanel.kt = PNL).  Plain pointers and sizes only: a JNI / Panama / ctypes
 * shim binds these symbols directly (INTEGRATION.md shows the Kotlin-side binding).
 *
 * Semantics are the reference's, bit for bit in IEEE binary64:
 *   - bodies are SoA fp64 arrays (x, y, vx, vy, m) in the caller's list order (BHA:21-25);
 *   - one bh_step() == one PhysicsEngine.step() (BHA:405-439): build, a(t), kick, drift,
 *     build, a(t+dt), kick, merge (BHA:463-532), so N may shrink;
 *   - the quadtree jitter (BHA:146-151) mutates positions exactly as the reference does;
 *   - bodies outside the root cell are not inserted but still integrate (BHA:126).
 *
 * Errors: every int-returning call returns 0 on success and a negative BH_E* code on
 * failure; bh_last_error() returns a human-readable message.  Nothing aborts the process.
 * Threading: one host thread per engine handle; calls are synchronous (results are
 * visible to bh_get_bodies on return), like step() under runBlocking (BHA:408,426).
 */
#ifndef BH_ENGINE_H
#define BH_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_OK 0
#define BH_E_INVALID (-1)  /* bad argument */
#define BH_E_DEVICE (-2)   /* HIP runtime error */
#define BH_E_COMM (-3)     /* RCCL error */
#define BH_E_CAPACITY (-4) /* caller buffer too small; *n_out holds the required size */
#define BH_E_STATE (-5)    /* call not valid in this state */

/* The Config.kt fields the hot path reads live, plus the merge knobs.
 * Replaces: Config.G (CFG:11), Config.DT (CFG:14), Config.theta (CFG:23),
 * Config.SOFT2 (CFG:20), Config.WIDTH_PX/HEIGHT_PX (CFG:5,8; root cell BHA:360-361),
 * PhysicsEngine.mergeMaxMass (BHA:315), PhysicsEngine.mergeMinDist (BHA:321). */
typedef struct bh_params {
    double G;
    double dt;
    double theta;
    double soft2;
    int32_t width_px;
    int32_t height_px;
    double merge_max_mass;
    double merge_min_dist;
} bh_params;

/* Reference defaults (CFG:5-23, BHA:315,321). */
void bh_default_params(bh_params *p);

typedef struct bh_engine bh_engine;

/* new PhysicsEngine(...) (BHA:287) on HIP device `device`, single GPU. */
int bh_create(const bh_params *p, int device, bh_engine **out);

/* new PhysicsEngine(...) (BHA:287) over every GPU of `device_mask` (bit d = HIP device d; 0 = every
 * visible device) behind ONE handle: the reference's step() fans its force evaluation out over
 * worker threads and joins them (computeAccelerations, BHA:374-395, inside runBlocking, BHA:408,
 * 426); this handle fans every step out over the GPUs and returns when all are done, so the one
 * PhysicsEngine object of the front-end (NBodyPanel.kt:103, 290-293) drives all of them.
 * Inside: one member engine per GPU -- the ranks of bh_create_dist's decomposition (replicated
 * state, locally essential tree builds, every exchange an in-place RCCL all-gather over xGMI on
 * communicators made in this process by ncclCommInitAll) -- each driven by its own host thread
 * (member 0 by the caller's).  Every call of this header takes the handle: calls that change the
 * state run on every member, calls that read it read member 0's replica (complete at every API
 * boundary), bh_set_mirror / bh_map_bodies use member 0's mirror.  One set bit = bh_create (the
 * pipelined one-GPU engine).  Results are bit-identical to bh_create's on the paths tested: one
 * GPU, members that share a device (device-to-device copies) and a one-rank RCCL communicator;
 * the distinct-device RCCL path (more than one rank) has not run on hardware yet, so callers
 * should keep one GPU (mask 1, or bh_create) unless they opt in (the Kotlin drop-in's default).
 * A call that fails on one member -- or whose waits for the others exceed BH_COMM_TIMEOUT_S
 * seconds (default 300; 0 = forever) -- aborts the others' waits (RCCL: ncclCommAbort) and returns
 * an error from every member; the handle then returns BH_E_COMM for every call that uses the
 * bodies until bh_reset_bodies, which makes new communicators. */
int bh_create_multi(const bh_params *p, uint32_t device_mask, bh_engine **out);

/* The same over an explicit device list, repeats allowed: a device listed twice hosts two members
 * (RCCL refuses two ranks per device), so a list with repeats -- or BH_MULTI_EXCHANGE=copy in the
 * environment -- exchanges by device-to-device copies between the members (an in-process group,
 * bh_create_local) instead of RCCL; the pieces, rounds and layout are the same. */
int bh_create_multi_list(const bh_params *p, const int32_t *devices, int32_t count,
                         bh_engine **out);

/* Members of a multi-device handle (1 for any other engine) and member `rank`'s own handle, for
 * diagnostics (per-rank timings, LET statistics, collective logs, bh_debug_inject on one rank).
 * Owned by the handle: never bh_destroy a member, and never bh_step one on its own (its peers
 * would wait for it).  A plain engine is its own member 0. */
int bh_multi_world(const bh_engine *e);
bh_engine *bh_multi_member(bh_engine *e, int rank);

/* Multi-rank engines log every collective they issue, in host issue order: 4 int64 per entry --
 * the engine's state-changing API call count when it was issued, the site (1 a round of
 * accelerations, 2 a round of new positions, 3 a round of velocities, 4 the LET cell tables,
 * 5 the end-of-call LET status all-reduce, 6 the settings check at creation), the bytes every
 * rank receives, and the stream (0 the engine's, 1 the exchange stream).  Every rank of a
 * decomposition must log the same sequence: RCCL pairs the n-th call of every rank.  The
 * in-process exchange logs the same entries.  BH_E_CAPACITY + *n_out if cap is too small. */
int bh_collective_log(const bh_engine *e, int64_t *out4, int64_t cap, int64_t *n_out);
int bh_collective_log_clear(bh_engine *e);

/* Multi-GPU member: one process per GPU; `unique_id` is the 128-byte RCCL id produced by
 * bh_comm_unique_id() on rank 0 and broadcast by the caller (e.g. torch.distributed).
 * Replaces computeAccelerations' fan-out over worker threads (BHA:374-395) by a fan-out over
 * GPUs.  Every rank holds a replica of the state and owns one contiguous range of the Hilbert
 * wave order (bh_shard_range).  Per force evaluation a rank either
 *   - builds a locally essential tree (from 2 ranks up, or BH_LET=1): only the depth-8 cells its
 *     bodies can open, plus the top computed from every rank's cell values (one all-gather of
 *     2 MB cell tables); it evaluates its range, kicks (and drifts) its own bodies, and the new
 *     positions -- 16 B per body -- are all-gathered over RCCL in BH_SHARD_ROUNDS rounds into
 *     every replica; velocities stay with their owners and are all-gathered before the next
 *     full build; or
 *   - builds the full tree (the first build after a reset, every 32 builds): it evaluates its
 *     range and the accelerations are all-gathered, after which every rank integrates every body.
 * At the end of every bh_step call the positions and velocities are complete on every rank
 * (velocities all-gathered if the call ended with a LET build); bh_get_quads then builds the
 * last build's full tree on demand (lastTree) without changing the rank's state.
 * The merge rule is replicated (identical inputs).  world == 1 with a non-NULL id runs the same
 * RCCL path on one rank (used to test it on one GPU).  BH_LET and BH_ROUND_FRACS must be equal
 * on every rank (checked at creation: BH_E_INVALID on every rank otherwise). */
int bh_create_dist(const bh_params *p, int device, int rank, int world, const void *unique_id,
                   bh_engine **out);
int bh_comm_unique_id(void *out128);

/* RCCL's own view of the engine's communicator: *nranks = ncclCommCount, *rank =
 * ncclCommUserRank; *nranks = 0 (and *rank = the engine's rank) for an engine without one
 * (single GPU, in-process group, solo). */
int bh_comm_ranks(const bh_engine *e, int32_t *nranks, int32_t *rank);

/* Test hooks.  what == 1: the next locally essential tree build of this rank trips the node
 * array guard (let.hip k_let_guard), as a broken invariant on one rank would; the call must then
 * be replayed by every rank of the group alike.  what == 2 + k (k < 98): the k-th next full tree
 * build (k = 0: the next one) raises the jitter replay's error flag, as the unsupported-geometry
 * guard would; the bh_step call whose step uses that tree returns BH_E_STATE -- for a call's last
 * pipelined build (the next call's first tree) that is the next call; what == 99: that carried tree
 * (one GPU, after a call) raises its flag now (BH_E_STATE if there is none).  what == 100 + k: this rank
 * fails host-side (BH_E_COMM) right before its k-th next collective; what == 200 + k: before its
 * k-th next in-process group barrier -- a rank-local error between collectives: every rank of the
 * decomposition must then return an error within a bounded time, refuse further calls with
 * BH_E_COMM, and step bit-exactly again after bh_reset_bodies. */
int bh_debug_inject(bh_engine *e, int what);

/* Progress of an engine, safe to read from any thread while a call runs (a watchdog's
 * heartbeat): out4[0] state-changing API calls begun, [1] collectives issued, [2] the site of
 * the last one (as bh_collective_log), [3] bit 0 a call is running, bit 1 the last multi-rank
 * call failed (BH_E_COMM until bh_reset_bodies), bit 2 its RCCL communicator was aborted.  A
 * multi-device handle reports member 0's (bh_multi_member for the others). */
int bh_progress(const bh_engine *e, int64_t *out4);

/* In-process rank group (testing the multi-GPU decomposition on one device, where RCCL refuses
 * several ranks): `world` engines of one process, each driven by its own host thread with
 * identical calls, exchange the force pieces with device-to-device copies on the same pieces,
 * rounds and in-place layout as bh_create_dist's ncclAllGather. */
typedef struct bh_local_group bh_local_group;
int bh_local_group_create(int world, bh_local_group **out);
void bh_local_group_destroy(bh_local_group *g);  /* after its members' bh_destroy */
int bh_create_local(const bh_params *p, int device, int rank, bh_local_group *group,
                    bh_engine **out);

/* Measurement only: rank `rank` of a `world`-rank engine running alone on one device -- the
 * rank's own work of a multi-GPU step (its locally essential tree builds, the traversal of its
 * pieces, the integration of every body) without peers and without the exchange: the peers'
 * bodies get zero acceleration and the cell values of the peers' cells come from the last
 * full build.  Times one GPU's share of the north-star decomposition on a single GPU; the
 * results are NOT the reference's. */
int bh_create_solo(const bh_params *p, int device, int rank, int world, bh_engine **out);

void bh_destroy(bh_engine *e);
const char *bh_last_error(const bh_engine *e);

/* Live Config mutation (PNL:247-260 change theta/DT/G between steps). */
int bh_set_params(bh_engine *e, const bh_params *p);
int bh_get_params(const bh_engine *e, bh_params *p);

/* PhysicsEngine.resetBodies(newBodies) (BHA:342-349): copy-in of n bodies. */
int bh_reset_bodies(bh_engine *e, int64_t n, const double *x, const double *y, const double *vx,
                    const double *vy, const double *m);

/* On-disk state (checkpoint / resume): the Config fields and the body list in the caller's
 * order as one little-endian file: an 80-byte header -- the 8-byte magic "BHSTATE1", a uint32
 * holding the size of the block that follows the first 16 bytes (64: the bh_params fields and
 * the int64 N), a uint32 flags word (0), that block -- then x[N], y[N], vx[N], vy[N], m[N] fp64
 * from byte 16 + 64 = 80 (layout in csrc/state_io.cpp).  A file whose length is not
 * 80 + 40 N is rejected (BH_E_INVALID) before anything is allocated.  Loading = bh_set_params
 * + bh_reset_bodies (resetBodies, BHA:342-349) of the saved list, so a resumed run is
 * bit-identical to an uninterrupted one.  The file is written to path.tmp, then renamed. */
int bh_save_state(bh_engine *e, const char *path);
int bh_load_state(bh_engine *e, const char *path);

/* k x PhysicsEngine.step() (BHA:405-439). */
int bh_step(bh_engine *e, int32_t k);

/* bh_step(e, k) on a thread of the engine's own, for a caller that overlaps its own work with
 * the call (the drop-in shim: NBodyPanel's tick, PNL:290-306, around step(), BHA:405-439).
 * Needs the two-buffer mirror (bh_set_mirror(e, 2)), else BH_E_STATE.  Until bh_step_end the
 * caller may only read the mirror it mapped before (bh_map_bodies: the call writes the other
 * buffer) and call bh_step_positions (bh_step, bh_reset_bodies, bh_set_params, bh_get_bodies,
 * bh_map_bodies, bh_set_mirror, bh_get_quads, bh_compute_accelerations, bh_compute_potential,
 * bh_compute_field, bh_compute_field_direct, bh_compute_force_error, bh_compute_field_grid,
 * bh_find_neighbors, bh_find_knn, bh_find_knn_bodies, bh_find_groups, bh_compute_radial_profile,
 * bh_compute_diagnostics and bh_render_bodies return BH_E_STATE); bh_step_end joins and returns bh_step's result (then
 * bh_last_removed, bh_map_bodies, ... as after bh_step).  bh_render_quads is refused in the same
 * way, as bh_get_quads is, and so are bh_set_tracers, bh_get_tracers and bh_render_tracers, and
 * bh_set_step_log, bh_get_step_log and bh_get_step_log_phi.
 * bh_step_positions blocks until the call's positions and masses are final -- on one GPU that is
 * once its last merge rule is done, before its last traversal; else when the call ends -- and
 * returns the mirror planes x, y, m of the list after the call (n_out bodies; the other buffer
 * than the one mapped before) and survivors[j], ascending: survivor j's index in the list before
 * the call (n_before bodies) -- the removals are the indices missing from it (bh_last_removed
 * after bh_step_end).  vx and vy of the same buffer are final only after bh_step_end +
 * bh_map_bodies.  With x, y and m all NULL it returns as soon as the survivors are known (their
 * copy runs ahead of the planes').  If the call fails, bh_step_positions returns its error; if it
 * fails after the hand-off (an unsupported jitter geometry), bh_step_end does. */
int bh_step_begin(bh_engine *e, int32_t k);
int bh_step_positions(bh_engine *e, const double **x, const double **y, const double **m,
                      const uint32_t **survivors, int64_t *n_out, int64_t *n_before);
int bh_step_end(bh_engine *e);

/* getBodies().size */
int64_t bh_num_bodies(const bh_engine *e);

/* PhysicsEngine.getBodies() (BHA:335) copy-out; any pointer may be NULL to skip it.
 * Returns BH_E_CAPACITY with *n_out = N if cap < N. */
int bh_get_bodies(bh_engine *e, double *x, double *y, double *vx, double *vy, double *m,
                  int64_t cap, int64_t *n_out);

/* getBodies() without a copy (BHA:335; NBodyPanel reads every body after every step,
 * PNL:302-306): a pinned host mirror of the bodies in the caller's list order.
 * bh_set_mirror(e, 1) makes every bh_step call write it itself -- positions and masses while
 * its last traversal still runs, velocities right after -- so the device-to-host copy overlaps
 * the call's last tree build.  bh_map_bodies waits for that copy (or makes one if the state
 * changed since) and returns pointers to x[N], y[N], vx[N], vy[N], m[N] (any pointer may be
 * NULL).  They stay valid -- and the data unchanged -- until the next call on this engine that
 * changes or moves the bodies (bh_step, bh_reset_bodies, bh_get_quads, bh_compute_accelerations,
 * bh_load_state, bh_set_mirror, bh_destroy).
 * bh_set_mirror(e, 2): two pinned buffers -- the calls write the one bh_map_bodies did not hand
 * out last, so the mapped bodies stay valid and unchanged until the next bh_map_bodies (or
 * bh_set_mirror, bh_destroy), and a caller may read them on one thread while a bh_step runs
 * on another (the drop-in compares its list against them during the step).  enabled is 0, 1
 * or 2 (else BH_E_INVALID). */
int bh_set_mirror(bh_engine *e, int enabled);
int bh_map_bodies(bh_engine *e, const double **x, const double **y, const double **vx,
                  const double **vy, const double **m, int64_t *n_out);

/* buildTree() + computeAccelerations() (BHA:359-395) on the current state, exactly as
 * the first half of step() does it (including the jitter's position mutation).  ax/ay
 * (length N, caller order) receive F/m.  visits (nullable, length N) receives the number
 * of non-empty nodes each body's traversal visited (accumulateForce calls passing the
 * mass == 0 test, BHA:216) — the V of the roofline byte model. */
int bh_compute_accelerations(bh_engine *e, double *ax, double *ay, int64_t *visits);

/* Per-body gravitational potential of the current state.  State semantics are exactly
 * bh_compute_accelerations': buildTree() as the first half of step() does it (the jitter's
 * position mutation included), then the evaluation; a tree-flag error is returned the same way.
 * Always a full build on this engine, never a locally essential tree, not sharded; on a
 * multi-device handle every member builds and member 0 evaluates and answers.
 * phi (length N, caller order; NULL keeps the result on the device): body b visits exactly the
 * nodes accumulateForce visits for it (BHA:215-239) -- mass-0 nodes skipped, its own leaf skipped
 * by identity, an internal node taken iff s2 < theta^2 * dist2 (strict) -- and every taken node,
 * in pre-order, adds
 *     dx = comX - b.x;  dy = comY - b.y;  r2 = dx*dx + dy*dy + soft2
 *     s += mass * (1.0 / sqrt(r2))          (IEEE sqrt and divide, no contraction, s from +0.0)
 * phi_b = -(G * s): bit-reproducible.  An accepted cell that contains b includes b's own mass,
 * as the force of that cell does (a self term -G m_b / sqrt(r2) that vanishes as theta -> 0); at
 * theta = 0 nothing is accepted and phi is the exact softened pair potential over the bodies in
 * the tree (an all-pairs kernel, bit-identical to the walk).  Bodies outside the root cell are
 * walked (they feel the tree) but are in nobody's sum. */
int bh_compute_potential(bh_engine *e, double *phi);

/* Conservation read-out, fp64 sums over every live body (out-of-root ones included). */
typedef struct bh_diagnostics {
    int64_t n;
    double mass;          /* sum m                          */
    double mx, my;        /* sum m*x, sum m*y               */
    double px, py;        /* sum m*vx, sum m*vy             */
    double lz;            /* sum m*(x*vy - y*vx)            */
    double kinetic;       /* sum 0.5*m*(vx*vx + vy*vy)      */
    double potential;     /* 0.5 * sum m*phi; 0 if not asked */
} bh_diagnostics;
/* with_potential = 0: reductions only, over the current state -- no build, no state change.
 * with_potential = 1: as bh_compute_potential (a build: the state semantics above), then the
 * reductions on the state after that build; phi stays on the device.
 * The sums run on the device in the caller's list order, per-workgroup partials in a fixed
 * order and one final workgroup, without floating-point atomics: two calls on the same state --
 * or two engines holding the same list -- return identical bits.  N = 0 returns all zeros. */
int bh_compute_diagnostics(bh_engine *e, int with_potential, bh_diagnostics *out);

/* HIP-event duration (ms) of the last potential kernel launch (bh_compute_potential, or
 * bh_compute_diagnostics with the potential); 0 before the first. */
int bh_potential_kernel_ms(const bh_engine *e, double *ms);

/* The field of the current state at n_probe points that are not bodies of it: acceleration and
 * potential at (px[j], py[j]).  The tree and the state semantics are exactly
 * bh_compute_potential's: buildTree() as the first half of step() does it (the jitter's position
 * mutation included), or the tree the previous call carried; always a full build on this engine,
 * never a locally essential tree, not sharded; a tree-flag error is returned the same way; on a
 * multi-device handle every member builds and member 0 evaluates and answers.  The probes never
 * enter the engine's state, its caller-order bookkeeping or its mirror: the call leaves what
 * bh_compute_accelerations would leave.
 * Probe j is a Body(px[j], py[j], 0, 0, pm[j]) that is not in the tree; pm = NULL gives every
 * probe mass 1.0, and (ax, ay) is then the field per unit mass (G * 1.0 and / 1.0 are exact).
 * It visits the nodes accumulateForce visits for such a body (BHA:215-239): mass-0 nodes are
 * skipped, EVERY non-empty leaf is taken -- nothing is skipped by identity, so a probe that sits
 * on a body gets that body's full term, m / sqrt(soft2) in the potential -- and an internal node
 * is taken iff s2 < theta^2 * dist2 (strict).  Every taken node, in pre-order, adds
 *     dx = comX - px;  dy = comY - py;  r2 = dx*dx + dy*dy + soft2
 *     invR = 1.0 / sqrt(r2);  invR2 = 1.0 / r2        (IEEE sqrt and divide, no contraction)
 *     f = G * pm * m * invR2                          (left to right, BHA:256)
 *     fx += f * dx * invR;  fy += f * dy * invR;  s += m * invR           (all from +0.0)
 * and ax = fx / pm, ay = fy / pm (BHA:390-391), phi = -(G * s): bit-reproducible, no
 * floating-point atomics, two calls with the same probes on the same state return identical
 * bits.  Nothing special-cases odd inputs -- the result is what this arithmetic gives: pm = 0
 * gives NaN accelerations and a valid phi, a probe on a centre of mass at soft2 = 0 gives NaN and
 * -inf, a NaN coordinate gives NaN.  Probes outside the root cell, far outside it or non-finite
 * are walked like any other.  With no body in the tree every sum stays +0.0 (phi = -0.0).
 * theta = 0 goes through the same walk, which then opens every node: O(n_probe x nodes); this
 * call has no tiled all-pairs kernel for probes -- bh_compute_field_direct (below) is that kernel,
 * at any theta.
 * ax, ay, phi (each nullable) have length n_probe, in the caller's probe order.  n_probe = 0
 * returns BH_OK after the build, launches nothing and leaves bh_field_kernel_ms as it was.
 * BH_E_INVALID (with bh_last_error text): e NULL, n_probe < 0 or > 2^28, px or py NULL with
 * n_probe > 0. */
int bh_compute_field(bh_engine *e, int64_t n_probe, const double *px, const double *py,
                     const double *pm, double *ax, double *ay, double *phi);

/* HIP-event duration (ms) of the last field kernel launch (bh_compute_field; the probes' keying,
 * sort and upload are outside it); 0 before the first. */
int bh_field_kernel_ms(const bh_engine *e, double *ms);

/* Which bodies of the current state lie within a radius of n_probe points: counts, the nearest
 * one, and the index lists.  The tree and the state semantics are exactly bh_compute_field's:
 * the build with its jitter or the carried tree, always a full build on this engine, never a
 * locally essential tree, not sharded; a tree-flag error is returned the same way; on a
 * multi-device handle every member builds and member 0 answers; the probes never enter the
 * engine's state: the call leaves what bh_compute_accelerations would leave.
 * The candidate set S is the leaf sequence of bh_compute_field_direct: every non-empty leaf that
 * lies under no mass-0 node.  So a body outside the root cell (or dropped from the tree by the
 * jitter, BHA:126) is never found, a mass-0 body is never found, and a negative-mass body under
 * a node of positive mass is found.
 * Probe j has the radius rj = pr[j], or r if pr is NULL (r is then not used).  Body b of S is a
 * neighbour of probe j iff
 *     rj >= 0 && dx*dx + dy*dy <= rj*rj,   dx = x_b - px[j];  dy = y_b - py[j]
 * in binary64, nothing fused, on the positions of the state after the call's build.  `<=` so that
 * r = 0 finds coincident bodies; nothing is skipped by identity (a probe on a body finds it with
 * d2 = 0); a NaN coordinate, or a NaN or negative radius in pr, finds nothing; +inf finds all of
 * S; probes outside the root cell, at 2^40 or at 1e300 are legal.
 *   count[j]       the number of neighbours of probe j;
 *   nearest[j]     the caller index of the neighbour smallest under the order (d2, caller index),
 *   d2_nearest[j]  and that d2 = dx*dx + dy*dy; -1 and +inf if there is none;
 *   indices[offsets[j] .. offsets[j + 1])  the neighbours' caller indices, ascending;
 *                  offsets[n_probe] and *n_total are the total.
 * Caller indices are indices into the list bh_get_bodies returns after the call.  count, nearest,
 * d2_nearest [n_probe] and n_total are each nullable; offsets [n_probe + 1] and indices [cap] are
 * given both or neither.  If cap is less than the total the call returns BH_E_CAPACITY with
 * count, nearest, d2_nearest, offsets and *n_total complete and indices untouched: one re-call
 * with cap >= *n_total suffices (the re-call builds again, as every call does: where that build's
 * jitter moves bodies once more, it answers for the state it leaves).  Lists of more than
 * 2^31 - 1 entries in all are refused (BH_E_INVALID): ask in batches.
 * Every output is an integer or a minimum under a total order -- no floating-point sum, no atomic
 * on a float: two calls, two engines holding the same list, or a multi-device handle return
 * identical bytes.  The walk prunes a cell by bh_neighbor_reach's bound (below), which changes
 * the work, never the result.
 * n_probe = 0 returns BH_OK after the build, launches nothing, leaves bh_neighbors_kernel_ms as
 * it was and sets *n_total = 0 (and offsets[0] = 0).  With no body in the tree every count is 0
 * and every offset 0.
 * BH_E_INVALID (with bh_last_error text): e NULL, n_probe < 0 or > 2^28, px or py NULL with
 * n_probe > 0, pr NULL and r NaN or negative, exactly one of offsets and indices given, cap < 0.
 * BH_E_STATE between bh_step_begin and bh_step_end. */
int bh_find_neighbors(bh_engine *e, int64_t n_probe, const double *px, const double *py,
                      double r, const double *pr, int64_t *count, int64_t *nearest,
                      double *d2_nearest, int64_t *offsets, int64_t *indices, int64_t cap,
                      int64_t *n_total);

/* HIP-event duration (ms) of the last bh_find_neighbors call's device work, from its first walk
 * to its last kernel (the scan of the counts, the second walk and the segmented sort included;
 * with lists it spans the host's read-back of the total between the two walks; the probes'
 * keying, sort and upload are outside it); 0 before the first. */
int bh_neighbors_kernel_ms(const bh_engine *e, double *ms);

/* The pruning bound of bh_find_neighbors' walk for the root cell of these params (host-only: no
 * device, no engine), returned by the function the kernel's host side itself uses (as
 * bh_launch_plan's values are).  *reach = D_d for 0 <= depth < 40: in any tree an engine with
 * this root cell can build, every body of S under a depth-d internal node lies within D_d of that
 * node's (comX, comY), provided the node's mass lies in [2^-900, 2^k) with 2^k the power of two
 * below DBL_MAX / (4 max |coordinate| of the root cell) -- the walk opens any other node
 * unconditionally.  D_d = 2 sqrt(2) h_d (the cell's diagonal) + a jitter allowance + the centre
 * of mass's rounding, all with a relative margin of 2^-40.
 * BH_E_INVALID: p or reach NULL, depth outside 0..39, params without a valid root cell. */
int bh_neighbor_reach(const bh_params *p, int32_t depth, double *reach);

/* The k nearest bodies of n_probe points (bh_find_knn) and of every body of the state
 * (bh_find_knn_bodies): bounded work per probe wherever it lies, where a fixed radius drowns in a
 * dense core and finds nothing in the tails.
 * The tree, the state semantics, the errors and the multi-device handle are exactly
 * bh_find_neighbors': the build with its jitter or the carried tree, always a full build, never
 * sharded; a tree-flag error is returned the same way; the call leaves what
 * bh_compute_accelerations would leave; on a multi-device handle every member builds and member 0
 * answers.
 * The candidate set S is bh_find_neighbors': every non-empty leaf under no mass-0 node.  Body b of
 * S is a candidate of probe j iff
 *     r_max >= 0 && dx*dx + dy*dy <= r_max*r_max,   dx = x_b - px[j];  dy = y_b - py[j]
 * in binary64, nothing fused, on the positions of the state after the call's build.  r_max = +inf
 * means no cap.  A NaN probe coordinate finds nothing; probes outside the root cell, at 2^40 or at
 * 1e300 are legal, and a d2 of +inf is a value like any other.  bh_find_knn skips nothing by
 * identity: a probe on a body finds it with d2 = 0.
 * Row j is the first min(k, candidates) candidates under the total order (d2, caller index):
 *   idx[j*k + i]   the caller index of the i-th nearest,
 *   d2[j*k + i]    and its d2 = dx*dx + dy*dy, in that order;
 *   found[j]       the number of entries; the tail of a shorter row holds -1 and +inf.
 * idx, d2 [n_probe * k] and found [n_probe] are each nullable.  Caller indices are indices into
 * the list bh_get_bodies returns after the call.  The row equals bh_find_neighbors' list for
 * r = r_max, sorted by (d2, index) and cut at k.
 * Every output is an integer or a d2 that one candidate's arithmetic produced -- no
 * floating-point sum, no atomic on a float: two calls, two engines holding the same list, or a
 * multi-device handle return identical bytes.  The walk prunes by bh_neighbor_reach's bound
 * around a radius that starts from a seed (an upper bound on the k-th distance taken from k real
 * candidates) and shrinks to the k-th best so far; both change the work, never the result
 * (DESIGN.md §20).
 * bh_find_knn_bodies: the probes are the N bodies of the list after the build, in caller order
 * (nothing is uploaded); row i belongs to caller index i.  A body's own leaf is skipped by
 * identity, so the rows hold the k nearest *other* bodies; a coincident other body is found with
 * d2 = 0.  A body that is not in S (outside the root cell, dropped by the jitter, or of mass 0) is
 * a probe like any other and skips nothing.  rows_cap is the room of the arrays in rows:
 * rows_cap < N returns BH_E_CAPACITY with *n_rows = N (nullable) and the arrays untouched; N = 0
 * returns BH_OK with *n_rows = 0.
 * n_probe = 0 returns BH_OK after the build, launches nothing and leaves bh_knn_kernel_ms as it
 * was.  With no body in the tree every found is 0 and every row is padding.
 * BH_E_INVALID (with bh_last_error text), before anything is launched: e NULL, n_probe < 0 or
 * > 2^28, px or py NULL with n_probe > 0, k outside 1..BH_KNN_MAX_K, r_max NaN or negative,
 * n_probe * k (or N * k) > 2^31 - 1 ("ask in batches"), a negative rows_cap.
 * BH_E_STATE between bh_step_begin and bh_step_end. */
#define BH_KNN_MAX_K 64
int bh_find_knn(bh_engine *e, int64_t n_probe, const double *px, const double *py, int32_t k,
                double r_max, int64_t *idx, double *d2, int64_t *found);
int bh_find_knn_bodies(bh_engine *e, int32_t k, double r_max, int64_t *idx, double *d2,
                       int64_t *found, int64_t rows_cap, int64_t *n_rows);

/* HIP-event duration (ms) of the last bh_find_knn / bh_find_knn_bodies call's device work, from
 * the seed kernel to the walk's last store (the leaf sequence and the probes' upload, keying and
 * sort are outside it); 0 before the first. */
int bh_knn_kernel_ms(const bh_engine *e, double *ms);

/* What the k-nearest walk launches for n_lane probes and lists of k entries (host-only: no
 * device, no engine; returned by the function the launch itself branches on, as
 * bh_direct_field_shape's values are): out4 = {lanes per wave, waves per workgroup, LDS bytes per
 * workgroup, workgroups}.  The waves per workgroup are the field walk's, halved until the
 * workgroup's lists (waves x 64 lanes x k entries of 12 bytes) fit 64 KiB.
 * BH_E_INVALID: out4 NULL, n_lane < 0 or > 2^28, k outside 1..BH_KNN_MAX_K. */
int bh_knn_shape(int64_t n_lane, int32_t k, int64_t *out4);

/* One group of bh_find_groups' catalogue. */
typedef struct bh_group {
    int64_t label;   /* smallest caller index among the group's members */
    int64_t count;   /* members */
    int64_t first;   /* members[first .. first + count) are this group's, ascending */
    double mass, mx, my, px, py;   /* fixed-order sums, below */
} bh_group;                        /* 64 bytes */

typedef struct bh_groups_summary {
    int64_t n_bodies;      /* N of the list after the call */
    int64_t n_in_tree;     /* |S| */
    int64_t n_groups_all;  /* components of S, singletons included */
    int64_t n_groups;      /* those with count >= min_members */
    int64_t largest_label; /* label of the group with the most members, the lower label on ties; -1 if S is empty */
    int64_t largest_count; /* 0 if S is empty */
} bh_groups_summary;

/* The friends-of-friends groups of the current state: two bodies are friends if they are no
 * farther apart than the linking length, a group is a connected component of that relation.
 * Which clumps exist, what each weighs and where it is, without copying the bodies out.
 * The tree and the state semantics are exactly bh_find_neighbors': the build with its jitter or
 * the carried tree, always a full build on this engine, never a locally essential tree, not
 * sharded; a tree-flag error is returned the same way; on a multi-device handle every member
 * builds and member 0 answers; the call leaves what bh_compute_accelerations would leave.
 * The candidate set S is bh_find_neighbors': the leaf sequence of bh_compute_field_direct, every
 * non-empty leaf that lies under no mass-0 node.  So a body outside the root cell (or dropped
 * from the tree by the jitter, BHA:126) and a mass-0 body are in no group, and a negative-mass
 * body under a node of positive mass is in S.
 * Bodies a != b of S are linked iff
 *     dx*dx + dy*dy <= link*link,   dx = x_a - x_b;  dy = y_a - y_b
 * in binary64, nothing fused, on the positions of the state after the call's build.  The relation
 * is symmetric bit for bit (x_a - x_b is the exact negation of x_b - x_a).  `<=` so that link = 0
 * links coincident bodies; +inf makes S one group.  A group is a connected component of the link
 * graph on S; its label is the smallest caller index among its members.  Caller indices are
 * indices into the list bh_get_bodies returns after the call.
 * Outputs, each nullable with its cap (an array that is NULL is not asked for, whatever its cap):
 *   label[i], i < N   the label of body i's group, or -1 for a body not in S; needs
 *                     label_cap >= N;
 *   members           the caller indices of S sorted by (label, caller index); needs
 *                     members_cap >= n_in_tree (N always suffices);
 *   groups            the groups with count >= min_members in ascending label, n_groups entries;
 *                     needs groups_cap >= n_groups; `first` indexes members and is valid whether
 *                     or not members was asked for;
 *   summary           always complete when the call returns BH_OK or BH_E_CAPACITY.
 * The sums of a group: its members in ascending caller index are c0 < c1 < ...; the term of
 * member c is m, m*x, m*y, m*vx, m*vy for mass, mx, my, px, py -- each one binary64 multiply,
 * never fused; x, y are the positions after the build, vx, vy the state's (a build does not touch
 * them).  Block k holds members [256k, 256k + 256) of that list; its partial is the sequential
 * sum of its terms in order from +0.0; the group's value is the sequential sum of the block
 * partials in order from +0.0.  No floating-point atomic is used anywhere.
 * Every output is an integer or such a sum: two calls, two engines holding the same list, or a
 * multi-device handle return identical bytes.  The walk prunes a cell by bh_neighbor_reach's
 * bound and the unions happen in whatever order the device runs them, which changes the work,
 * never the result.
 * If a given array's cap is too small the call returns BH_E_CAPACITY with summary complete and
 * all three arrays untouched: one re-call with sufficient caps suffices (it builds again, as
 * every call does: where that build's jitter moves bodies once more, it answers for the state it
 * leaves).
 * N = 0, or S empty: BH_OK, summary all zero (n_bodies too) except largest_label = -1, and
 * bh_groups_kernel_ms left as it was; with bodies but an empty S the labels are all -1.  (With
 * N = 0 nothing is launched; an empty S is found out on the device, whose kernels then idle.)
 * Cost: the walk visits every friend of every body as a leaf, like bh_find_neighbors, so a call
 * costs O(linked pairs); a linking length far above the mean separation of a dense scene is slow.
 * Accepting a whole cell at once where its reach is small against link is left out on purpose
 * (DESIGN.md §18), and so are unbinding, per-group angular momentum and groups of tracers.
 * BH_E_INVALID (with bh_last_error text): e NULL, link NaN or negative, min_members < 1, a
 * negative cap.  BH_E_STATE between bh_step_begin and bh_step_end. */
int bh_find_groups(bh_engine *e, double link, int64_t min_members,
                   int64_t *label,   int64_t label_cap,
                   int64_t *members, int64_t members_cap,
                   bh_group *groups, int64_t groups_cap,
                   bh_groups_summary *summary);

/* HIP-event duration (ms) of the last bh_find_groups call's own device work, from the link
 * walk's start to the last catalogue kernel (the build, the leaf sequence and the copy-out are
 * outside it); 0 before the first call that found a non-empty S. */
int bh_groups_kernel_ms(const bh_engine *e, double *ms);

/* One annulus of bh_compute_radial_profile. */
typedef struct bh_radial_bin {      /* 64 bytes */
    int64_t count;                  /* selected bodies with edges[k] <= R < edges[k+1] */
    double mass;                    /* sum m                    */
    double mr;                      /* sum m*R                  */
    double mvr, mvt;                /* sum m*vr, sum m*vt       */
    double mvr2, mvt2;              /* sum (m*vr)*vr, sum (m*vt)*vt */
    double lz;                      /* sum m*w                  */
} bh_radial_bin;

typedef struct bh_radial_summary {  /* 48 bytes */
    int64_t n_bodies;    /* N of the list */
    int64_t n_selected;  /* N, or the number of distinct indices in subset */
    int64_t n_binned;    /* selected bodies that fell into a bin */
    int64_t n_inner;     /* selected, R < edges[0] */
    int64_t n_outer;     /* selected, R >= edges[n_bin] (R = +inf included) */
    int64_t n_nan;       /* selected, R is NaN */
} bh_radial_summary;

#define BH_RADIAL_MAX_BINS 4096
/* The bodies of the current state in annuli about a centre: per bin the count and the sums from
 * which the surface density, the rotation curve, the velocity dispersions and the enclosed mass
 * of a disk follow, without copying the bodies out.  The centre (cx, cy) and the frame velocity
 * (cvx, cvy) are the caller's -- a group's mx / mass, my / mass, px / mass, py / mass from
 * bh_find_groups, for instance, with that group's members as the subset.
 * State and errors as bh_compute_diagnostics(e, 0, ...): no build, no jitter, no state change; the
 * call reads the state the caller sees (what bh_get_bodies returns now), never the jittered
 * positions of a tree the engine built ahead, and covers every live body of the list: bodies
 * outside the root cell and bodies of mass 0 or of negative mass are in.  A multi-device handle
 * answers from member 0's replica.
 * Selection.  subset == NULL: every body (n_subset is ignored).  Else the set of the caller
 * indices subset[0 .. n_subset): a duplicate counts once, n_subset = 0 selects nothing.  Indices
 * refer to the list bh_get_bodies returns now.
 * The terms of body c, in binary64, every operation separate, never fused:
 *     dx = x - cx;  dy = y - cy;  R2 = dx*dx + dy*dy;  R = sqrt(R2)        (IEEE sqrt)
 *     ux = vx - cvx;  uy = vy - cvy
 *     u = dx*ux + dy*uy;  w = dx*uy - dy*ux
 *     vr = u / R;  vt = w / R        (IEEE divide);  if R2 == 0.0: vr = vt = +0.0
 *     terms: m, m*R, m*vr, m*vt, (m*vr)*vr, (m*vt)*vt, m*w
 * R2 == 0 is the one special case (the natural centre is the central body's own position, and 0/0
 * would poison bin 0); nothing else is: a non-finite centre or frame velocity, a coordinate of
 * 1e300 and a NaN coordinate give what this arithmetic gives.
 * Bins.  edges[0 .. n_bin] are strictly increasing, edges[0] >= 0; edges[n_bin] may be +inf.
 * Body c is in bin k iff edges[k] <= R && R < edges[k+1]: the lower edge is inclusive and the
 * compare is on R itself.  R < edges[0] counts in n_inner, R >= edges[n_bin] (an R of +inf even
 * under a last edge of +inf) in n_outer, a NaN R is in no bin and counts in n_nan.
 * Sums.  Bin k's selected members in ascending caller index are c0 < c1 < ...; block j holds
 * members [256j, 256j + 256) of that list, its partial is the sequential sum of its terms in that
 * order from +0.0, and the bin's value is the sequential sum of its block partials in order from
 * +0.0 -- bh_group's rule with the bin as the label.  No floating-point atomic is used anywhere:
 * two calls, two engines holding the same list, or a multi-device handle return identical bytes.
 * An empty bin is all zeros (+0.0).
 * Outputs: bins (n_bin records) and summary are each nullable; with both NULL the call validates
 * its arguments and launches nothing.  N = 0: BH_OK, all zeros, nothing launched and
 * bh_radial_profile_kernel_ms left as it was.
 * Left out on purpose: tracers as the population, per-bin azimuthal harmonics and
 * a profile per group in one call.
 * BH_E_INVALID (with bh_last_error text), before anything is launched: e NULL, edges NULL, n_bin
 * outside 1..BH_RADIAL_MAX_BINS, an edge that is NaN, edges[0] < 0, edges not strictly increasing,
 * subset non-NULL with n_subset < 0 or > 2^28, a subset index outside [0, N).  BH_E_STATE between
 * bh_step_begin and bh_step_end. */
int bh_compute_radial_profile(bh_engine *e, double cx, double cy, double cvx, double cvy,
                              int32_t n_bin, const double *edges,        /* n_bin + 1 */
                              const int64_t *subset, int64_t n_subset,   /* NULL: every body */
                              bh_radial_bin *bins,                       /* n_bin, nullable */
                              bh_radial_summary *summary);               /* nullable */

/* HIP-event duration (ms) of the last bh_compute_radial_profile call's own device work, from the
 * staging of the state in list order to the last emit kernel (the uploads of edges and subset
 * and the copy-out are outside it); 0 before the first call that launched anything. */
int bh_radial_profile_kernel_ms(const bh_engine *e, double *ms);

/* n_bin + 1 bin edges from r_min to r_max (host-only, no handle).  Linear:
 *     edges[k] = r_min + (r_max - r_min) * ((double)k / (double)n_bin),  0 < k < n_bin
 * log_spacing != 0 (needs r_min > 0):
 *     edges[k] = r_min * exp2(log2(r_max / r_min) * k / n_bin)          (the host's libm)
 * with edges[0] = r_min and edges[n_bin] = r_max exact in both.
 * BH_E_INVALID: edges NULL, n_bin outside 1..BH_RADIAL_MAX_BINS, r_min not finite or negative
 * (or not positive with log_spacing), r_max <= r_min, NaN or +inf, a result that is not strictly
 * increasing (bins narrower than the spacing of binary64 there). */
int bh_radial_edges(double r_min, double r_max, int32_t n_bin, int log_spacing, double *edges);

/* The exact field of the current state at n_probe points: bh_compute_field with no cell ever
 * accepted, whatever the engine's theta.  Arguments, probe semantics (a probe is not in the tree;
 * pm = NULL is mass 1.0; nothing is skipped by identity; nothing special-cases odd inputs),
 * nullable outputs, n_probe = 0 (BH_OK after the build, nothing launched,
 * bh_direct_field_kernel_ms left as it was), the 2^28 cap, the BH_E_INVALID cases and the state
 * semantics (the build with its jitter or the carried tree, tree-flag errors, never sharded; on a
 * multi-device handle every member builds and member 0 evaluates and answers) are
 * bh_compute_field's.  Every non-empty leaf that lies under no mass-0 node adds, in pre-order,
 * the terms written out there: the result is bit-identical to bh_compute_field on an engine that
 * holds the same state with theta = 0.  It is computed by an LDS-tiled all-pairs kernel over the
 * tree's leaf sequence (direct_field.hip) instead of that walk: O(n_probe x leaves), the sum of
 * one probe sequential, the probes in parallel.  With no body in the tree every sum stays +0.0. */
int bh_compute_field_direct(bh_engine *e, int64_t n_probe, const double *px, const double *py,
                            const double *pm, double *ax, double *ay, double *phi);

/* The force accuracy of the tree at the engine's theta, on sampled bodies, in one call with one
 * build.  State semantics are exactly bh_compute_accelerations': buildTree() with its jitter or
 * the carried tree, then the normal evaluation of every body (sharded on a multi-rank engine; on
 * a multi-device handle every member evaluates and member 0 does the rest); a tree-flag error is
 * returned the same way.  idx[j] (j < n_sample) is an index into the current list, the one
 * bh_get_bodies returns: any order, duplicates allowed.
 *   ax_tree[j], ay_tree[j]   what bh_compute_accelerations returns for body idx[j] now;
 *   ax_exact[j], ay_exact[j] what it would return on an engine holding the same state with
 *     theta = 0: the sum over every non-empty leaf of that same tree but the body's own (skipped
 *     by identity), in pre-order, by the all-pairs kernel of bh_compute_field_direct.  A body
 *     outside the root cell has no leaf and is summed like a probe of its own mass; a body of
 *     mass 0 gets NaN (fx / 0 is not special-cased).
 * The summary is made on the host, in idx order, in binary64 without contraction:
 *   rel_j = sqrt(dx*dx + dy*dy) / sqrt(ex*ex + ey*ey),  dx = ax_tree[j] - ax_exact[j], dy alike,
 *   ex = ax_exact[j], ey = ay_exact[j]; sample j is used iff its four values are finite and the
 *   denominator is > 0; mean_rel = (sequential sum of rel_j) / n_used; rms_rel = sqrt((sequential
 *   sum of rel_j * rel_j) / n_used).
 * The four arrays (length n_sample) and out are each nullable.  n_sample = 0 builds and
 * evaluates, launches no all-pairs kernel and returns an all-zero out with worst = -1.
 * BH_E_INVALID (with bh_last_error text) before anything is launched: e NULL, n_sample < 0 or
 * > 2^28, idx NULL with n_sample > 0, an idx[j] outside [0, N). */
typedef struct bh_force_error {
    int64_t n_sample;
    int64_t n_used;   /* samples whose four accelerations are finite and |a_exact| > 0 */
    int64_t worst;    /* position in idx[] of max_rel (first on ties); -1 if n_used == 0 */
    double max_rel, mean_rel, rms_rel;   /* of |a_tree - a_exact| / |a_exact|; 0 if n_used == 0 */
} bh_force_error;
int bh_compute_force_error(bh_engine *e, int64_t n_sample, const int64_t *idx,
                           double *ax_tree, double *ay_tree, double *ax_exact, double *ay_exact,
                           bh_force_error *out);

/* HIP-event duration (ms) of the last k_direct_targets launch (bh_compute_field_direct or
 * bh_compute_force_error; uploads, the leaf sequence and the sample gather are outside it); 0
 * before the first. */
int bh_direct_field_kernel_ms(const bh_engine *e, double *ms);

/* The launch shape of k_direct_targets for n_target targets: out3 = {leaf records per LDS tile,
 * lanes per workgroup, targets per lane}.  Host-only: no device, no handle; returned by the
 * function the launch itself branches on (as bh_launch_plan's values are).  Up to 32 768 targets
 * {256, 64, 1}: one-wave workgroups, so that a few thousand targets spread over the part; above,
 * {1024, 256, 2}.  BH_E_INVALID: out3 NULL or n_target < 0. */
int bh_direct_field_shape(int64_t n_target, int64_t *out3);

/* The field of the current state on a regular grid, made on the device: the potential map under a
 * frame.  Nothing is uploaded but the six grid values, no point is keyed or sorted, and the
 * results land in row-major planes without a permutation.
 * Grid point (c, r), 0 <= c < nx, 0 <= r < ny, is the probe
 *     Body(x0 + (double)c * dx, y0 + (double)r * dy, 0, 0, 1.0)
 * -- each coordinate one multiply and one add in binary64, never fused -- that is not in the tree.
 * ax, ay, phi (each nullable) are row-major ny x nx planes: index r * nx + c holds, bit for bit,
 * what bh_compute_field returns for that coordinate with pm = NULL on the same state.  Everything
 * else is bh_compute_field's, unchanged: every non-empty leaf is taken (a grid point on a body gets
 * that body's full term), the criterion is strict, the terms are added in pre-order, nothing
 * special-cases odd inputs, and points outside the root cell -- at 2^40 or at 1e300 -- are walked
 * like any other.  Zero and negative spacings are legal: the arithmetic decides.  With no body in
 * the tree every sum stays +0.0 (phi = -0.0).
 * The tree, the state semantics and the errors are exactly bh_compute_field's: the build with its
 * jitter or the carried tree, always a full build, never sharded; tree-flag errors returned the
 * same way; the call leaves what bh_compute_accelerations would leave; on a multi-device handle
 * every member builds and member 0 evaluates and answers; BH_E_STATE between bh_step_begin and
 * bh_step_end.
 * stats (nullable) is computed on the device from the three planes alone, by a fixed-order
 * reduction without floating-point atomics; extremes are taken under the order (value, row-major
 * index), zeros comparing equal by value (the sign of a zero extreme is unspecified).  With all
 * three planes NULL and stats non-NULL the call still evaluates, and nothing comes to the host but
 * the struct: where the deepest well in view is and what range a colour map should span.
 * BH_E_INVALID (with bh_last_error text): e or g NULL, nx or ny outside 1..16384,
 * nx * ny > 1 << 24, a non-finite x0, y0, dx or dy. */
typedef struct bh_field_grid {
    double x0, y0;     /* world coordinates of grid point (column 0, row 0) */
    double dx, dy;     /* spacing along a row / between rows, world units   */
    int32_t nx, ny;    /* columns, rows: 1..16384 each, nx*ny <= 1<<24      */
} bh_field_grid;
typedef struct bh_field_grid_stats {
    int64_t n_phi;       /* grid points whose phi is finite */
    int64_t i_phi_min;   /* row-major index of phi_min, first on ties; -1 if n_phi == 0 */
    double phi_min, phi_max;   /* over those points; 0 if n_phi == 0 */
    int64_t n_acc;       /* points whose ax and ay are both finite */
    int64_t i_a2_max;    /* row-major index of a2_max, first on ties; -1 if n_acc == 0 */
    double a2_max;       /* max of ax*ax + ay*ay (binary64, not contracted); 0 if n_acc == 0 */
} bh_field_grid_stats;
int bh_compute_field_grid(bh_engine *e, const bh_field_grid *g, double *ax, double *ay,
                          double *phi, bh_field_grid_stats *stats);

/* HIP-event duration (ms) of the last k_field_grid launch (bh_compute_field_grid; the stats
 * reduction and the copy-out are outside it); 0 before the first.  No other call changes it. */
int bh_field_grid_kernel_ms(const bh_engine *e, double *ms);

/* The launch shape of k_field_grid for an nx x ny grid: out4 = {tile columns, tile rows, waves per
 * workgroup, tiles}.  One wave is one compact tile of grid points: 8 x 8, halved alternately
 * (8 x 4, 4 x 4, 4 x 2, ...) while the grid has too few points to fill the part with full waves;
 * the tiles are numbered along a Z-order curve over the tile grid.  Host-only: no device, no
 * handle; returned by the function the launch itself branches on (as bh_direct_field_shape's
 * values are).  BH_E_INVALID: out4 NULL, nx or ny outside 1..16384, nx * ny > 1 << 24. */
int bh_field_grid_shape(int32_t nx, int32_t ny, int64_t *out4);

/* The body pass of a frame, rasterised on the device: what NBodyPanel.paintComponent's loop over
 * engine.getBodies() paints (PNL:302-307) -- one pixel per body, black if m >= 1000 (PNL:303),
 * white otherwise, a later body of the list overwriting an earlier one -- returned as an image
 * instead of five N-long planes. */
typedef struct bh_view {
    double view_x, view_y;   /* NBodyPanel.viewX / viewY (world coords of the screen origin) */
    double zoom;             /* NBodyPanel.zoom: finite, > 0 */
    int32_t width, height;   /* panel size in pixels: 1..16384 each, width*height <= 1<<24 */
    double heavy_mass;       /* PNL:303 colour threshold; bh_default_view sets 1000.0 */
} bh_view;
/* view_x = view_y = 0, zoom = 1.0, Config WIDTH_PX x HEIGHT_PX (2400 x 800, CFG:5,8), 1000.0 */
void bh_default_view(bh_view *v);
/* pixels, owner, counts: row-major height x width planes; any of them may be NULL.
 * Exactly PNL:302-307 over the list bh_get_bodies would return.  For body i in caller order
 *     tx = (x_i - view_x) * zoom;  ty = (y_i - view_y) * zoom             (binary64)
 *     sx = toInt(tx);  sy = toInt(ty)       (Kotlin's Double.toInt(): NaN gives 0, otherwise
 *                                            truncation toward zero, saturating at the Int range)
 * and the body is drawn iff 0 <= sx < width && 0 <= sy < height -- equivalently tx is NaN or
 * -1 < tx < width, and the same for ty (the test is made in double, before any conversion).
 * Truncation is not floor: a body up to one pixel left of or above the view lands in column or
 * row 0, and so does a NaN coordinate, as in the reference.
 *   owner[p]   the largest caller index drawn on pixel p (the body that painted last);
 *              0xFFFFFFFF where nothing was drawn
 *   pixels[p]  0 nothing, 1 white (m[owner] < heavy_mass), 2 black (m[owner] >= heavy_mass)
 *   counts[p]  the number of bodies drawn on p (the reference has no such plane: the density a
 *              renderer wants at a million bodies)
 * Every output is a function of the list alone (integer max and integer add, no floating-point
 * atomics): two calls, or two engines holding the same list, return identical bytes.
 * State and errors as bh_compute_diagnostics(e, 0, ...): no build, no jitter, no state change;
 * the call reads the state the caller sees (never the jittered positions of a tree the pipelined
 * engine built ahead) and writes only buffers of its own, allocated on first use and kept while
 * the view size is unchanged.  A multi-device handle answers from member 0's replica, as
 * bh_get_bodies does.  N = 0: pixels and counts all 0, owner all 0xFFFFFFFF.
 * BH_E_INVALID (with bh_last_error text): NULL e or v; zoom not finite or <= 0; heavy_mass NaN;
 * width or height outside 1..16384 or width*height > 1<<24.  BH_E_STATE between bh_step_begin
 * and bh_step_end. */
int bh_render_bodies(bh_engine *e, const bh_view *v, uint8_t *pixels, uint32_t *owner,
                     uint32_t *counts);

/* HIP-event duration (ms) of the last bh_render_bodies' two kernels (rasterise + resolve); 0
 * before the first (a call with N = 0 launches nothing and leaves it as it was). */
int bh_render_kernel_ms(const bh_engine *e, double *ms);

/* The grid of bh_compute_field_grid that lies under a view: one grid point per cell_px x cell_px
 * block of the view's pixels, at the block's centre.  Host-only.
 *     nx = ceil(width / cell_px);  ny = ceil(height / cell_px);  dx = dy = cell_px / zoom
 *     x0 = view_x + (0.5 * cell_px) / zoom;  y0 = view_y + (0.5 * cell_px) / zoom
 * BH_E_INVALID: v or g NULL, a view bh_render_bodies would refuse (same text), cell_px outside
 * 1..16384.  The call has no handle: after it returned BH_E_INVALID, bh_last_error(NULL) on the
 * same thread returns its text (until then, and after a success, "null engine" as ever). */
int bh_field_grid_of_view(const bh_view *v, int32_t cell_px, bh_field_grid *g);

/* Tracers: massless test particles stepped with the bodies -- points that feel the system, exert
 * nothing on it and are integrated by the same leapfrog, on the same trees, in the same bh_step
 * call (the restricted N-body experiment: two massive disks plus 10^6 tracers that draw the tails).
 * The engine holds a second list of n_tracer tracers (x, y, vx, vy) in binary64, in the caller's
 * order, independent of the body list.  Tracer t is a Body(x, y, vx, vy, 1.0) that is never
 * inserted into any tree -- the reference's body outside the root cell, "not inserted but walked
 * and integrated" (BHA:126), anywhere in the plane.  In every PhysicsEngine.step() that bh_step
 * runs, with `root` the tree the bodies use for that evaluation (after its jitter):
 *     (fx, fy) = root.accumulateForce(t)  -- exactly bh_compute_field's terms for pm = NULL:
 *                massless nodes skipped, EVERY non-empty leaf taken, an internal node taken iff
 *                s2 < theta^2 * dist2 (strict), terms added in pre-order from +0.0,
 *                f = (G * 1.0) * m * invR2;  ax = fx / 1.0;  ay = fy / 1.0
 *     first evaluation:   vx += ax * dtHalf;  vy += ay * dtHalf;  x += vx * dt;  y += vy * dt
 *     second evaluation:  vx += ax * dtHalf;  vy += ay * dtHalf        (BHA:412-432, never fused)
 * Tracers never take part in the merge rule: never victims, never heavy, not counted in N.
 * Nothing special-cases odd inputs: NaN and 1e300 coordinates give what the arithmetic gives; with
 * no body in the tree every sum is +0.0, the tracers drift on straight lines, and -0.0 + 0.0 turns
 * a -0.0 velocity into +0.0.  At theta = 0 the bodies use the all-pairs kernel and the tracers the
 * same walk, which then opens every node (bit-identical, as bh_compute_field documents; there is
 * no tiled tracer kernel).  A tracer's result does not depend on n_tracer, on its position in the
 * list, on the internal lane order or on how steps are grouped into calls (k steps in one call =
 * k one-step calls), and the bodies' results are bit for bit what they are without tracers.
 *
 * bh_set_tracers replaces the whole list (vx, vy nullable: zeros; n = 0 clears it and frees its
 * buffers).  BH_E_INVALID: e NULL, n < 0 or n > 2^28, x or y NULL with n > 0.  BH_E_STATE with
 * n > 0 on any engine that is not the one-GPU engine -- bh_create_dist, bh_create_local and
 * bh_create_solo engines and a multi-device handle with more than one member: their steps shard
 * their builds as locally essential trees, which a tracer cannot walk (bh_last_error says so);
 * n = 0 is accepted everywhere.
 * The list persists across bh_reset_bodies, bh_set_params and bh_load_state; it is not written by
 * bh_save_state (the BHSTATE1 format is unchanged) and not touched by any bh_compute_*,
 * bh_get_quads or bh_render_* call: only bh_step, bh_step_begin / bh_step_end and bh_set_tracers
 * change it.  bh_step(e, 0) leaves it alone.  After bh_step_end the tracers are final;
 * bh_step_positions says nothing about them.  A call replayed for a merge mailbox overflow steps
 * them exactly once.
 * bh_get_tracers: copy-out in list order, any plane nullable; BH_E_CAPACITY with *n_out =
 * n_tracer if cap < n_tracer.  bh_num_tracers: -1 for a NULL handle. */
int bh_set_tracers(bh_engine *e, int64_t n, const double *x, const double *y, const double *vx,
                   const double *vy);
int64_t bh_num_tracers(const bh_engine *e);
int bh_get_tracers(bh_engine *e, double *x, double *y, double *vx, double *vy, int64_t cap,
                   int64_t *n_out);

/* Average HIP-event duration (ms) of the tracer walks of the last bh_step call and their number
 * (two per step), as bh_traverse_kernel_ms reports the traversals.  Taken only while
 * bh_set_profiling(e, 1) -- otherwise *launches = 0 and no event is recorded; the walks are then
 * also counted under phase [1] of bh_last_timings. */
int bh_tracer_kernel_ms(const bh_engine *e, double *avg_ms, int64_t *launches);

/* The launch shape of the tracer walk for n_tracer tracers: out3 = {tracers per wave, waves per
 * workgroup, R}.  The first two are bh_compute_field's for as many probes; R is the number of
 * steps between re-orderings of the lane map (lane q walks tracer order[q]; the map is the
 * tracers' order along the build's Morton curve, made by bh_set_tracers and re-made every R steps
 * before the step's first walk -- results do not depend on it).  Host-only: no device, no handle;
 * returned by the function the launch itself branches on (as bh_direct_field_shape's values are).
 * BH_E_INVALID: out3 NULL, n_tracer < 0 or > 2^28. */
int bh_tracer_launch_shape(int64_t n_tracer, int64_t *out3);

/* The tracer pass of a frame: bh_render_bodies' pixel rule over the tracer list (the toInt rule;
 * drawn iff t is NaN or -1 < t < size; the later list index wins).  owner[p] is the largest tracer
 * index drawn on p, 0xFFFFFFFF where nothing was drawn; counts[p] the number of tracers drawn on
 * p; either may be NULL.  The view is checked as by bh_render_bodies (same BH_E_INVALID cases and
 * bh_last_error text; heavy_mass is checked but not used); state semantics are bh_render_bodies':
 * no build, no state change, BH_E_STATE between bh_step_begin and bh_step_end.  n_tracer = 0:
 * owner all 0xFFFFFFFF, counts all 0. */
int bh_render_tracers(bh_engine *e, const bh_view *v, uint32_t *owner, uint32_t *counts);

/* The step log: the conservation read-out of every step, made inside bh_step -- the energy-drift
 * curve of a run from inside the pipelined k-step call, without one-step calls and without a
 * separate potential walk per step.  While the log is on, every PhysicsEngine.step() that bh_step
 * runs appends one record to a ring on the device; nothing waits for the host and nothing is
 * copied per step; bh_get_step_log reads the ring out in one copy.
 * One record describes the state after the step's second kick (BHA:432) and before its merge rule
 * (BHA:438) -- positions and velocities both at t + dt, the only instant of a step at which kinetic
 * and potential energy belong together -- in its own terms, because a re-build would jitter again:
 *   root   the tree of the step's second evaluation (BHA:426), after that build's jitter;
 *   L      the reference's body list at BHA:432: bodies removed by earlier steps -- earlier steps
 *          of the same call included -- are gone, the order is what removeAt leaves;
 *   phi_b  for every body b of L exactly what bh_compute_potential defines over root:
 *          accumulateForce's nodes, mass-0 nodes skipped, the own leaf skipped by identity, an
 *          internal node taken iff s2 < theta^2 * dist2 (strict), the terms mass * (1.0 / sqrt(r2))
 *          in IEEE arithmetic added in pre-order from +0.0, phi_b = -(G * s); a body outside the
 *          root cell walks.  The sum rides in the step's own second traversal (the force's point
 *          blocks hold 1 / sqrt(r2) already); at theta = 0 it is the all-pairs kernel's;
 *   d      what bh_compute_diagnostics' reduction returns for the six planes x, y, vx, vy, m, phi
 *          of L in list order: the same partition by |L|, the same fixed trees, no floating-point
 *          atomics; d.n = |L|, d.potential = 0.5 * sum m phi.
 * So a step that neither jitters nor merges logs, bit for bit, what bh_compute_diagnostics(e', 1, .)
 * returns after the same step on a twin engine.  The records do not depend on how steps are
 * grouped into calls (k steps in one call = k one-step calls, removals included), on the lane map,
 * the mirror, tracers or profiling, and the log changes nothing else: bodies, tracers, removals
 * and every other output of bh_step are bit for bit what they are with the log off.
 *
 * bh_set_step_log: capacity 0 turns the log off and frees its buffers; 1..1<<20 makes a ring of
 * that many records, empty, with step and t back at 0.  The ring overwrites its oldest record.
 * The log persists across bh_reset_bodies, bh_set_params and bh_load_state, step and t running on
 * (dt is read per call, as bh_step reads it); it is not written by bh_save_state.  bh_step(e, 0)
 * logs nothing; with N = 0 a step logs an all-zero d, step and t advancing.  A call replayed for
 * a merge mailbox overflow logs each step once; a bh_step that returns an error empties the ring
 * and puts step and t back to their values before the call.  Steps of a bh_step_begin call are
 * logged like any others; until bh_step_end the two getters and bh_set_step_log return BH_E_STATE.
 * BH_E_INVALID: e NULL, capacity outside 0..1<<20.  BH_E_STATE with capacity > 0 on any engine
 * that is not the one-GPU engine -- bh_create_dist, bh_create_local and bh_create_solo engines and
 * a multi-device handle with more than one member: a locally essential tree is no full tree, and
 * no walk of one gives a body its full potential (bh_last_error says so); 0 is accepted everywhere.
 * bh_get_step_log: the ring oldest first, *n_out = min(records logged, capacity) of them;
 * BH_E_CAPACITY + *n_out if cap is too small.  bh_get_step_log_phi: the phi plane of the newest
 * record in the order of its L, d.n entries; BH_E_CAPACITY + *n_out likewise; BH_E_STATE if no step
 * was logged since the log was enabled or since the last bh_reset_bodies / bh_load_state; with the
 * log off, *n_out = 0.  Both: BH_E_INVALID for e or n_out NULL, or the array NULL with cap > 0. */
typedef struct bh_step_record {
    int64_t step;        /* 1, 2, ...: steps logged since bh_set_step_log enabled the log */
    double t;            /* sum of those steps' dt, added in binary64 in step order from +0.0 */
    bh_diagnostics d;    /* the state after the step's second kick, before its merge rule */
} bh_step_record;
int bh_set_step_log(bh_engine *e, int64_t capacity);
int bh_get_step_log(bh_engine *e, bh_step_record *out, int64_t cap, int64_t *n_out);
int bh_get_step_log_phi(bh_engine *e, double *phi, int64_t cap, int64_t *n_out);

/* Average HIP-event duration (ms) of the log's own kernels per step of the last bh_step call --
 * the staging into list order and the reduction, not the walk, which bh_traverse_kernel_ms times --
 * and their number (one per step), as bh_tracer_kernel_ms reports the tracer walks: taken only
 * while bh_set_profiling(e, 1), otherwise *launches = 0; counted under phase [2] of
 * bh_last_timings. */
int bh_step_log_kernel_ms(const bh_engine *e, double *avg_ms, int64_t *launches);

/* Indices (into the list as it was before the last bh_step call, ascending) of the bodies the
 * merge rule removed during that call — what a shim needs to apply BHA:519's removeAt to the
 * caller's own list and keep Body identity.  BH_E_CAPACITY + *n_out if cap is too small. */
int bh_last_removed(const bh_engine *e, int64_t *idx, int64_t cap, int64_t *n_out);

/* getTreeForDebug().visitQuads{} (BHA:265-274,329-332): pre-order list of every cell
 * (cx, cy, h) of the last tree, or of a freshly built one if the cache was dropped
 * (after resetBodies or a merge, BHA:348,526).  BH_E_CAPACITY + *n_out if cap too small. */
int bh_get_quads(bh_engine *e, double *cx, double *cy, double *h, int64_t cap, int64_t *n_out);

/* The quadtree overlay of a frame, rasterised on the device: what NBodyPanel.paintComponent draws
 * for getTreeForDebug().visitQuads (key D, PNL:326-344), returned as one plane of line-draw counts
 * instead of a list of cells.  Nothing of the tree is copied to the host.
 * For every cell q that bh_get_quads would return (BHA:265-274), in binary64 with Kotlin's
 * Double.toInt() (NaN gives 0, otherwise truncation toward zero, saturating at the Int range):
 *     x = toInt(((q.cx - q.h) - view_x) * zoom)
 *     y = toInt(((q.cy - q.h) - view_y) * zoom)
 *     s = toInt(q.h * 2.0 * zoom)
 * and the panel draws drawLine(x, y, x, y + s) and drawLine(x, y, x + s, y) (PNL:335-339):
 * one-pixel lines, end points included, clipped to width x height.
 *   lines[p]   (row-major height x width) the number of those line draws that cover pixel p; a
 *              cell's corner pixel counts 2.  The panel draws with a translucent colour (alpha 180,
 *              PNL:330): what it shows at p is that colour composited lines[p] times, so the
 *              count is the complete picture and does not depend on the order of the cells.
 *              NULL: only the count is produced and no image work is launched.
 *   *n_quads   (nullable) the number of cells: bh_get_quads' *n_out.  N = 0 gives 1, the root.
 * x + s and y + s are formed in 64-bit integers.  That equals the reference wherever Kotlin's Int
 * addition does not overflow -- it cannot for the panel's zoom range 1..10 (PNL:56-57) with the
 * view clamped to the world (PNL:121-128); where it would, the contract is the unwrapped line.
 * Truncation is not floor: a cell edge up to one pixel left of or above the view lands in column
 * or row 0, and so does a NaN view origin, as for bh_render_bodies.
 * State and errors are exactly bh_get_quads': the tree is the last tree (lastTree, BHA:435; the
 * copy a pipelined call kept aside included), or, if the cache was dropped, a freshly built one
 * whose jitter moves the bodies as getTreeForDebug's does; on a multi-rank engine the lazy full
 * build; a multi-device handle prepares on every member and answers from member 0.
 * bh_render_quads then bh_get_quads (or the other way round) leaves the same state and sees the
 * same cells as two bh_get_quads calls.  bh_render_quads returns BH_E_STATE between bh_step_begin
 * and bh_step_end.  The view is checked as by bh_render_bodies (same BH_E_INVALID cases and
 * bh_last_error text; heavy_mass is checked but not used); NULL e or v: BH_E_INVALID.
 * Integer adds only: two calls, two engines holding the same tree, or a multi-device handle
 * return identical bytes.  Working buffers are the call's own, allocated on first use and kept
 * while the view size is unchanged. */
int bh_render_quads(bh_engine *e, const bh_view *v, uint32_t *lines, int64_t *n_quads);

/* HIP-event duration (ms) of the last bh_render_quads' kernels (cells + the two scans, or the
 * counting kernel alone when lines was NULL); 0 before the first. */
int bh_render_quads_kernel_ms(const bh_engine *e, double *ms);

/* Per-phase device timings (ms) of the last bh_step call, summed over its steps:
 * [0] tree build, [1] traversal, [2] integration, [3] merge, [4] all-gather. */
int bh_last_timings(const bh_engine *e, double *out5);

/* Number of tree nodes (non-empty + skip slots) of the last build; for byte models. */
int64_t bh_last_tree_nodes(const bh_engine *e);

/* Traversal kernel timing for roofline: average duration (ms) of the force-evaluation
 * kernel over the launches of the last bh_step, measured with HIP events on the
 * engine's own stream; *launches receives the count. */
int bh_traverse_kernel_ms(const bh_engine *e, double *avg_ms, int64_t *launches);

/* The same measurement per launch, in launch order (ms): min / median / max of the traversal
 * over a timed region.  BH_E_CAPACITY + *n_out if cap is too small. */
int bh_traverse_kernel_samples(const bh_engine *e, double *ms, int64_t cap, int64_t *n_out);

/* Lane efficiency of the last bh_compute_accelerations(..., visits != NULL): the sum over
 * bodies of visited nodes, the sum over wavefronts of nodes the wave's shared cursor stopped
 * at (union of its 64 bodies' traversals), and the number of wavefronts. */
int bh_traversal_stats(const bh_engine *e, int64_t *lane_visits, int64_t *wave_iters,
                       int64_t *waves);

/* All counters of the last bh_compute_accelerations(..., visits != NULL), summed over bodies /
 * wavefronts: [0] nodes visited, [1] point-force contributions (accepted internal nodes and
 * other bodies' leaves: the 20-flop work units of the FP64 roofline), [2] nodes the wavefronts'
 * shared cursors stopped at, [3] point-force blocks the wavefronts executed, [4] wavefronts.
 * Lane efficiency = [0] / (64 [2]); force-block lane use = ([1] + bodies) / (64 [3]). */
int bh_traversal_counters(const bh_engine *e, int64_t *out5);

/* Multi-rank build sharding (locally essential tree): out5[0] LET builds, out5[1] full-tree
 * builds since the engine was created, out5[2] bodies in the largest LET subset of the last
 * bh_step call (the cells this rank's bodies can open), out5[3] node records of the last LET
 * tree, out5[4] bh_step calls replayed because a subset outgrew its capacity (the capacity
 * follows the previous call's subsets, so the build needs no host round trip).  LET builds run
 * on every multi-rank engine (2 ranks up); BH_LET=1 in the environment before creating an engine
 * enables them also on one rank, BH_LET=0 keeps every build full. */
int bh_let_stats(const bh_engine *e, int64_t *out5);

/* Enable/disable per-phase event timing (default off: no events in the hot loop). */
int bh_set_profiling(bh_engine *e, int enabled);

/* Multi-GPU force evaluation runs in BH_SHARD_ROUNDS rounds.  Rank r owns the contiguous
 * lanes [r * rounds * sub, (r + 1) * rounds * sub) of the Hilbert wave order (one spatial
 * region: its locally essential tree has one halo), and round k evaluates its lanes
 * [lo, hi) = [(r * rounds + k) * sub, + sub) clipped to n, with sub = ceil(n / (world * rounds))
 * rounded up to whole wavefronts.  The accelerations of lane q are written to the exchange
 * buffer at bh_gather_slot(n, world, q) = (k * world + r) * sub + i (q = (r * rounds + k) * sub
 * + i): the pieces of round k are adjacent there and are all-gathered in place (one
 * ncclAllGather per round) on a second stream while round k + 1 is evaluated.  Host-only; used
 * by the engine itself. */
#ifndef BH_SHARD_ROUNDS
#define BH_SHARD_ROUNDS 4
#endif
int bh_shard_range(int64_t n, int rank, int world, int round, int64_t *lo, int64_t *hi);
int64_t bh_gather_slot(int64_t n, int world, int64_t lane);

/* The kernels and launch shapes that the one-GPU step picks from the list size alone, read out
 * for a fresh engine with these parameters after bh_reset_bodies(n) (capacity = n).  Host-only:
 * no device, no handle.  Each value is returned by the function that the tree build or the
 * traversal itself branches on, so the read-out moves with the code; tests take their sizes from
 * where it changes.  out receives min(cap, BH_PLAN_FIELDS) values, *n_out = BH_PLAN_FIELDS;
 * n = 0: all zero.  The build's fields describe every build after an engine's first (which has
 * no splitters yet and sorts with the library's radix sort).  BH_PLAN_NODE_ADDR64 describes every
 * tree walk of that engine, the queries' included: 0 while its node array (32 bytes a record)
 * stays below 4 GiB and a 32-bit byte offset reaches every record.  An engine's capacity never
 * shrinks, so one that once held a longer list keeps the form of that list. */
enum {
    BH_PLAN_SMALL_FRONT = 0, /* 1: the build's front (keys, sort, prefix lengths) is one workgroup */
    BH_PLAN_SMALL_FRONT_P,   /* its sort width, the next power of two >= n (0: front is off)      */
    BH_PLAN_CELL_DEPTH,      /* D0, the depth of the cell-start table                              */
    BH_PLAN_SORT_BUCKETS,    /* buckets of the adaptive bucket sort                                */
    BH_PLAN_COM_CHUNKS,      /* centre-of-mass chunks (workgroups of the node emission)           */
    BH_PLAN_SPAN_GROUPS,     /* groups of chunk boundaries (above 1: the top span pass runs)      */
    BH_PLAN_OWN_SCAN,        /* 1: the build's own scan of the node counts, 0: the library's      */
    BH_PLAN_BFS,             /* 1: the step's first walk (kick and drift) is breadth first         */
    BH_PLAN_BFS_BITS,        /* node indices its bitmap covers (a larger tree: cursor walk)       */
    BH_PLAN_BPW,             /* first walk: bodies per wave                                        */
    BH_PLAN_WPB,             /* first walk: waves per workgroup                                    */
    BH_PLAN_XCD_GROUPS,      /* first walk: whole groups of workgroups remapped across the XCDs   */
    BH_PLAN_KICK_BPW,        /* kick-only walk: bodies per wave                                    */
    BH_PLAN_KICK_WPB,        /* kick-only walk: waves per workgroup                                */
    BH_PLAN_KICK_XCD_GROUPS, /* kick-only walk: whole remapped groups (the tail is not remapped)  */
    BH_PLAN_ORDER_RUNS,      /* runs of waves that a wave order would permute (0: too many)       */
    BH_PLAN_NODE_ADDR64,     /* 1: the walks fetch node records by a 64-bit address (array >= 4 GiB) */
    BH_PLAN_FIELDS
};
int bh_launch_plan(const bh_params *p, int64_t n, int64_t *out, int64_t cap, int64_t *n_out);

/* Diagnostic: checks, on HIP device `device`, the traversal's reduced-range exact sequences
 * for sqrt(d2), 1/sqrt(d2) and 1/d2 (traverse.hip) bit-for-bit against the IEEE operations on
 * n generated operands (random, near powers of two, near perfect squares, physical range);
 * on the first 2^26 of them it also evaluates the walk's opening criterion in its two forms
 * (s2 < theta^2 * d2 and d2 >= threshold) for several root cells and theta, every depth, d2 at
 * the threshold +- 2 ulp and random, and counts disagreements into the same number;
 * *mismatches receives the number of differing results (0 expected). */
int bh_selftest_fast_math(int device, int64_t n, uint64_t seed, int64_t *mismatches);

/* Block until all device work of this engine is complete. */
int bh_synchronize(bh_engine *e);

/* ---- scene generation (BodyFactory.kt = BF), host-side, deterministic -------------
 * Kotlin's kotlin.random.Random(seed) XorWow stream (kotlin-stdlib 2.2.20) restated so
 * that seeded scenes are reproducible; caller provides arrays of length n_total. */
int bh_scene_galaxy_disk(int32_t n_total, double eps_m2, double phi0, double bar_taper_r,
                         double radial_scale, double speed_jitter, double radial_jitter,
                         int32_t clockwise, int64_t seed, double vx, double vy, double x,
                         double y, double r, double min_r, double central_mass,
                         double total_satellite_mass, double G, double *ox, double *oy,
                         double *ovx, double *ovy, double *om);
int bh_scene_kepler_disk(int32_t n_total, int32_t clockwise, double radial_jitter,
                         double speed_jitter, int64_t seed, double vx, double vy, double x,
                         double y, double r, double G, double *ox, double *oy, double *ovx,
                         double *ovy, double *om);
int bh_scene_uniform(int32_t n, double m, int64_t seed, int32_t width_px, int32_t height_px,
                     double *ox, double *oy, double *ovx, double *ovy, double *om);

/* ---- fp32 3-D all-pairs engine: the physics of the reference's OpenGL compute shader
 * (gpu/GPU.kt:101-152 = "GPU").  a_i = sum_{j!=i} (G m_j) d / (d.d +
 * softening^2)^{3/2} with the hardware reciprocal square root (GLSL inversesqrt, GPU:140),
 * then v += a dt, x += v dt (GPU:145-146) — double-buffered instead of the reference's
 * in-place race.  fp32 throughout; parity is a tolerance, not bit-identity. */
typedef struct bh_nbody3d bh_nbody3d;
int bh_nbody3d_create(int device, bh_nbody3d **out);
void bh_nbody3d_destroy(bh_nbody3d *h);
const char *bh_nbody3d_last_error(const bh_nbody3d *h);
/* upload (replaces GpuNBody's SSBO upload of Body{x,y,z,vx,vy,vz,m}) */
int bh_nbody3d_set(bh_nbody3d *h, int64_t n, const float *x, const float *y, const float *z,
                   const float *vx, const float *vy, const float *vz, const float *m);
/* GpuNBody.simulate(dt, g, softening) x k (GPU:411-422) */
int bh_nbody3d_step(bh_nbody3d *h, int32_t k, float dt, float G, float softening);
/* one evaluation of the accelerations of the current state (no integration) */
int bh_nbody3d_accelerations(bh_nbody3d *h, float G, float softening, float *ax, float *ay,
                             float *az);
int bh_nbody3d_get(const bh_nbody3d *h, float *x, float *y, float *z, float *vx, float *vy,
                   float *vz, float *m, int64_t cap, int64_t *n_out);
/* GpuNBodyRenderer.computeCenterOfMass() (GPU:390-411) without its read-back of the body buffer:
 * out4 = sum x*m, sum y*m, sum z*m, sum m over the current bodies, accumulated in fp64 from the
 * fp32 state by a fixed-order device reduction (no floating-point atomics: the same state gives
 * the same bits).  The centre of mass is out4[0..2] / out4[3], (0, 0, 0) when out4[3] is 0. */
int bh_nbody3d_center_of_mass(bh_nbody3d *h, double out4[4]);
/* device time (ms) of the last bh_nbody3d_step / bh_nbody3d_accelerations call */
double bh_nbody3d_last_ms(const bh_nbody3d *h);

#ifdef __cplusplus
}
#endif
#endif /* BH_ENGINE_H */
