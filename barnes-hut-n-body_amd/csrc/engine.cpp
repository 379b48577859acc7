// Engine host code and the C-ABI (include/bh_engine.h).
//
// Replaces PhysicsEngine (BHA:287-532).  The engine owns the body state in HBM as SoA fp64
// arrays in Morton ("slot") order plus each body's caller-list index (cidx), the tree
// workspace, and one HIP stream.  A step is the reference's step() (BHA:405-439) as a fixed
// kernel sequence on that stream; the only host round trip is the merge rule's (BHA:463-532)
// candidate mailbox, and only while heavy bodies exist.
//
// Multi-GPU (bh_create_dist): every rank holds a replica of the state and owns one contiguous
// range of the Hilbert wave order.  The build is sharded: each rank builds a locally essential
// tree (let.hip) -- the cells its bodies may open, plus the top assembled from every rank's cell
// values (one all-gather of the cell tables) -- evaluates its range, kicks (and drifts) its own
// bodies in the traversal's epilogue, and the new positions (16 B per body) are all-gathered in
// place with RCCL over xGMI; velocities stay with their owners until the next full build, before
// which they are all-gathered.  Every BH_LET_REFRESH builds, after a reset and for the last build
// of every bh_step call (lastTree, BHA:435) the full tree is built by every rank; its
// accelerations are all-gathered and every rank integrates every body.  The merge rule is
// replicated (identical inputs, identical outcome) and needs no exchange.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "bh_device.hpp"
#include "bh_engine.h"
#include "multi.hpp"
#include "open_threshold.hpp"
#include "render_quads.hpp"
#include "render_view.hpp"

using namespace bh;

namespace {
constexpr int kPhases = 5;  // build, traverse, integrate, merge, allgather
}  // namespace

namespace bh {
void set_error(bh_engine *e, const std::string &msg);  // for the C-ABI's other translation units
}

// In-process rank group (bh_local_group_*): `world` engines of one process, one host thread
// each, that exchange the force pieces through device-to-device copies instead of RCCL -- the
// same pieces, rounds and in-place layout as the ncclAllGather path, so the multi-rank
// decomposition runs on one GPU (RCCL refuses several ranks per device).
//
// Every wait has a way out (the reference's join always returns, BHA:408, 426): a member whose
// call fails aborts the group (abort()), which wakes every member waiting in barrier() and makes
// every later barrier return false, until the members' bh_reset_bodies (reset()); a barrier that
// waits longer than BH_COMM_TIMEOUT_S aborts the group itself.
namespace {
// seconds a multi-rank engine waits for its peers (a barrier, a collective on the device) before
// it gives up and aborts (BH_COMM_TIMEOUT_S; 0 = forever)
double comm_timeout_s() {
    static const double t = [] {
        const char *v = std::getenv("BH_COMM_TIMEOUT_S");
        return v ? std::atof(v) : 300.0;
    }();
    return t;
}
}  // namespace

struct bh_local_group {
    int world = 0;
    std::vector<bh_engine *> members;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    std::atomic<bool> aborted{false};
    bool timed_out = false;  // (under mu) the abort came from a barrier's deadline
    // false: the group was aborted (before or while this member waited)
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (aborted.load()) return false;
        const uint64_t gen = generation;
        if (++arrived == world) {
            arrived = 0;
            ++generation;
            cv.notify_all();
            return true;
        }
        auto pred = [&] { return generation != gen || aborted.load(); };
        const double t = comm_timeout_s();
        if (t > 0.0) {
            if (!cv.wait_for(lk, std::chrono::duration<double>(t), pred)) {
                timed_out = true;
                aborted.store(true);
                cv.notify_all();
                return false;
            }
        } else {
            cv.wait(lk, pred);
        }
        return generation != gen;
    }
    void abort() {
        std::lock_guard<std::mutex> lk(mu);
        aborted.store(true);
        cv.notify_all();
    }
    // every member's bh_reset_bodies after an abort (no member waits: their calls have returned)
    void reset() {
        std::lock_guard<std::mutex> lk(mu);
        if (!aborted.load()) return;
        arrived = 0;
        ++generation;
        timed_out = false;
        aborted.store(false);
    }
};

// The kernel stopwatch of a query (bh_*_kernel_ms): two events around its last launch, made on
// first use.  `timed` is set once both were recorded; a failed call leaves the last reading.
struct Stopwatch {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
    int start(bh_engine *e, hipStream_t s);
    int stop(bh_engine *e, hipStream_t s);
    int ms(double *out) const;  // 0.0 before the first launch
    void destroy();
};

struct bh_engine {
    bh::Multi *multi = nullptr;  // a multi-device handle (multi.cpp): the members do the work
    // ... or, for a body list below multi_min bodies, one pipelined single-GPU engine on the first
    // device (like the reference's min(cores, n) workers, BHA:377): a step of a few 1e5 bodies is
    // launch-bound, and splitting it only adds launches and exchanges
    bh_engine *one = nullptr;
    bool use_one = false;
    int64_t multi_min = 0;
    bh_params p{};
    Geometry geo{};
    int device = 0;
    hipStream_t stream = nullptr;
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    bh_local_group *group = nullptr;             // in-process ranks (test path), or RCCL:
    hipStream_t comm_stream = nullptr;            // all-gathers, overlapping the next round
    // odd rounds' traversals: at 8 ranks a round is under one dispatch generation of waves, so
    // consecutive rounds run concurrently on two streams instead of each waiting for the tail
    hipStream_t stream2 = nullptr;
    hipEvent_t built_ev = nullptr;
    hipEvent_t round_ev[BH_SHARD_ROUNDS] = {};   // round k's forces written (compute stream)
    hipEvent_t gathered_ev = nullptr;            // every round gathered (comm stream)

    int64_t n = 0;     // live bodies
    int64_t cap = 0;   // allocated bodies
    int J_alloc = -1;  // J the node array was sized for

    BodyState st{};   // current state, slot (Morton) order
    BodyState alt{};  // second buffer: build / compaction target, copy-out staging
    double *a2 = nullptr;  // interleaved accelerations (slot order), 2 * chunk * world
    double *ax = nullptr, *ay = nullptr;  // caller-order copy-out staging

    uint64_t *keys = nullptr, *keys_s = nullptr;
    uint32_t *keys32 = nullptr, *keys32_s = nullptr;
    uint32_t *idx = nullptr, *perm = nullptr;
    uint32_t *perm2 = nullptr;  // the pipelined step's overlapped build's permutation
    int8_t *cpl = nullptr;
    uint32_t *cnt = nullptr, *base = nullptr;
    uint32_t *cell_start = nullptr;
    Node *nodes = nullptr;
    size_t node_cap = 0;
    uint32_t *span_list = nullptr, *super_list = nullptr;
    bh::SpanSlot *span_children = nullptr;
    uint32_t *scalars = nullptr;  // [1] tree error flags
    uint32_t *visits32 = nullptr;
    uint32_t *contrib32 = nullptr;     // per-body point-force contributions (diagnostics)
    uint32_t *wave_iters = nullptr;  // per-wave union of visited nodes (diagnostics)
    uint32_t *wave_blocks = nullptr; // per-wave point-force blocks executed (diagnostics)
    int64_t stat_lane_visits = 0, stat_wave_iters = 0, stat_waves = 0;
    int64_t stat_lane_contrib = 0, stat_wave_blocks = 0;

    // merge
    uint32_t *heavy = nullptr;
    uint32_t *keep = nullptr, *pos = nullptr;
    MergePair *box = nullptr;  // candidate pairs: header + pairs
    uint32_t box_cap = 0;
    uint32_t box_need = 0;     // pairs a step needed beyond the capacity (grown on retry)
    BodyState snap{};          // state at the start of a bh_step call (exact merge retry)
    int64_t snap_cap = 0, snap_n = 0;
    uint32_t *dlog = nullptr;        // removal log of the running bh_step call (caller indices)
    uint32_t *dead_sorted = nullptr; // the log sorted, for the compaction's renumbering
    uint64_t *rkeys = nullptr;       // replay sort scratch (long candidate lists)
    uint32_t *ridx = nullptr;
    uint32_t *mbits = nullptr;       // victim bitmap over caller indices (long lists)
    uint32_t *mslot = nullptr;       // caller index -> slot of the victims
    int64_t dlog_cap = 0;
    bool heavy_possible = true;  // false once a step saw no heavy body (heavies never appear)
    // the last build listed the heavy bodies in its order (heavy, count in scalars[14]): the merge
    // rule that follows it needs no k_heavy pass (the pipelined step's second build)
    bool heavy_ready = false;
    bool heavy_dirty = false;  // scalars[14] may be nonzero (a list no merge rule consumed)
    bool merge_ran = false;      // the running bh_step call launched the merge rule
    std::vector<int64_t> removed;  // removals of the last bh_step call, ascending (BHA:519)
    void *pin = nullptr;  // pinned staging for small read-backs (coherent: kernels write it too)
    void *pin_dev = nullptr;
    size_t pin_bytes = 0;

    void *scratch = nullptr;
    size_t scratch_bytes = 0;

    // adaptive bucket sort (tree_build.hip): splitters written by every build
    uint64_t *spl = nullptr;
    uint32_t *bcount = nullptr, *bstart = nullptr;
    uint32_t spl_nb = 0;  // splitters of the last build; 0 = none (next build sorts with rocprim)

    // theta = 0 all-pairs path (direct.hip), allocated on first use
    uint8_t *leaf_flags = nullptr;
    uint32_t *leaf_sel = nullptr, *leaf_count = nullptr;
    int32_t *leaf_cover = nullptr;  // 2 (node_cap + 1): subtrees of massless nodes
    LeafList leaves{nullptr};
    void *leaf_tmp = nullptr;
    size_t leaf_tmp_bytes = 0;
    size_t leaf_node_cap = 0;  // node capacity the flags were sized for
    int64_t leaf_cap = 0;

    // potential and global diagnostics (potential.hip), allocated on first use
    double *phi = nullptr;        // the last bh_compute_potential's phi, slot order
    int64_t phi_cap = 0;
    double *diag_part = nullptr;  // the reductions' workgroup partials, then their 8 results
    Stopwatch pot_sw;             // around the last potential kernel launch

    // bh_compute_field (field.hip): the call's own probe buffers, allocated on first use and
    // grown when needed; nothing of the engine's state or bookkeeping is kept here
    double *fld_in = nullptr;    // px, py, pm planes of fld_cap probes
    double *fld_out = nullptr;   // ax, ay, phi planes, by probe index
    uint32_t *fld_u32 = nullptr; // key, sorted key, index, order planes
    void *fld_scratch = nullptr;
    size_t fld_scratch_bytes = 0;
    int64_t fld_cap = 0;
    Stopwatch fld_sw;  // around the last field kernel

    // bh_compute_field_direct / bh_compute_force_error (direct_field.hip): the targets' buffers,
    // the calls' own as bh_compute_field's are, allocated on first use and grown when needed
    double *dfl_in = nullptr;         // tx, ty, tm planes of dfl_cap targets
    double *dfl_out = nullptr;        // ax, ay, phi, ax_tree, ay_tree planes, by target index
    uint32_t *dfl_u32 = nullptr;      // the samples' caller indices, their slots
    uint32_t *dfl_slot_of = nullptr;  // caller index -> slot, dfl_slot_cap entries
    int64_t dfl_cap = 0, dfl_slot_cap = 0;
    Stopwatch dfl_sw;  // around the last k_direct_targets launch

    // bh_compute_field_grid (field.hip k_field_grid): result planes of its own, allocated on
    // first use and kept while nx * ny does not grow; there is nothing to upload
    double *fgr_out = nullptr;                 // ax, ay, phi planes of fgr_cap grid points
    bh_field_grid_stats *fgr_stats = nullptr;  // the reduction's partials, then its result
    int64_t fgr_cap = 0;
    Stopwatch fgr_sw;  // around the last k_field_grid launch

    // bh_find_neighbors (neighbors.hip): the call's own buffers, allocated on first use and grown
    // when needed -- per probe (nbr_cap) and per list entry (nbr_list_cap)
    double *nbr_in = nullptr;      // px, py, pr planes of nbr_cap probes
    uint32_t *nbr_u32 = nullptr;   // key, sorted key, index, order planes
    int64_t *nbr_i64 = nullptr;    // count, offsets (nbr_cap + 1 each), nearest
    double *nbr_d2 = nullptr;      // d2_nearest
    void *nbr_scratch = nullptr;   // the probes' sort and the counts' scan
    size_t nbr_scratch_bytes = 0;
    int64_t nbr_cap = 0;
    uint32_t *nbr_idx = nullptr;   // the lists as written and as sorted, nbr_list_cap each
    int64_t *nbr_list = nullptr;   // ... and as int64, for the copy-out
    int64_t nbr_list_cap = 0;
    void *nbr_sort = nullptr;      // the segmented sort's scratch
    size_t nbr_sort_bytes = 0;
    Stopwatch nbr_sw;  // from the first walk to the last kernel of the last call
    // bh_find_knn / bh_find_knn_bodies (knn.hip): the calls' own buffers, allocated on first use
    // and grown when needed -- per uploaded probe (knn_cap), per lane (knn_lane_cap) and per row
    // entry (knn_row_cap)
    double *knn_in = nullptr;      // px, py planes of knn_cap probes
    uint32_t *knn_u32 = nullptr;   // key, sorted key, index, order planes
    void *knn_scratch = nullptr;   // the probes' sort
    size_t knn_scratch_bytes = 0;
    int64_t knn_cap = 0;
    double *knn_seed = nullptr;    // every lane's starting radius^2
    int64_t *knn_found = nullptr;
    int64_t knn_lane_cap = 0;
    int64_t *knn_idx = nullptr;    // the rows: k entries per lane
    double *knn_d2 = nullptr;
    int64_t knn_row_cap = 0;
    Stopwatch knn_sw;  // from the seed kernel to the walk's last store
    // bh_find_groups (groups.hip): the call's own buffers, allocated on first use and grown when
    // the list outgrows them (grp_cap bodies)
    uint32_t *grp_u32 = nullptr;   // parent, minc, rootof, val, val_s; flag, gid, first, keep, kidx
    uint64_t *grp_u64 = nullptr;   // key, sorted key
    int64_t *grp_i64 = nullptr;    // label, members; the summary
    double *grp_part = nullptr;    // the blocks' partial sums
    bh_group *grp_groups = nullptr;
    void *grp_scratch = nullptr;   // the sort and the scans
    size_t grp_scratch_bytes = 0;
    int64_t grp_cap = 0;
    // from the link walk to the last catalogue kernel of the last call that found a non-empty S;
    // a call records into grp_sw_run and the two change places once it knows S is not empty
    Stopwatch grp_sw, grp_sw_run;
    // bh_set_tracers (field.hip k_tracer_step): the tracer list and its lane map.  Nothing is
    // allocated while the list is empty; every buffer is sized for exactly trc_n tracers and made
    // anew when the count changes (a stale lane map would index past the planes)
    double *trc = nullptr;        // x, y, vx, vy planes of trc_n tracers, list order
    double *trc_snap = nullptr;   // the same at the start of a bh_step call that may be replayed
    uint32_t *trc_u32 = nullptr;  // key, sorted key, index, order planes
    void *trc_scratch = nullptr;
    size_t trc_scratch_bytes = 0;
    int64_t trc_n = 0, trc_snap_n = 0;
    int trc_age = 0, trc_snap_age = 0;  // steps walked with the current lane map
    double trc_ms_sum = 0.0;            // the tracer walks of the last bh_step call (profiling)
    int64_t trc_launches = 0;

    // bh_set_step_log (step_log.hip): a device ring of slog_cap records (0: off, nothing allocated)
    // and buffers of its own, sized for slog_bcap bodies: the logged walk's phi by slot, the six
    // planes x, y, vx, vy, m, phi of the last logged step in list order (never e->alt: the pipelined
    // step is using it), the survivors' index and the reduction's partials.  Everything the host
    // needs for a record -- its ring slot, step and t -- it knows when it enqueues the step
    void *slog_ring = nullptr;
    int64_t slog_cap = 0;
    int64_t slog_head = 0;   // records written since the ring was last emptied (slot = head % cap)
    int64_t slog_step = 0;   // steps logged since bh_set_step_log enabled the log
    double slog_t = 0.0;     // their dt, added in step order
    int64_t slog_call_head = 0, slog_call_step = 0;  // at the start of the running bh_step call
    double slog_call_t = 0.0;                        // (a replay and a failed call go back there)
    double *slog_phi = nullptr, *slog_stage = nullptr, *slog_part = nullptr;
    uint32_t *slog_keep = nullptr, *slog_pos = nullptr;
    void *slog_tmp = nullptr;
    size_t slog_tmp_bytes = 0;
    int64_t slog_bcap = 0;
    bool slog_phi_valid = false;  // slog_stage holds the planes of the ring's newest record
    double slog_ms_sum = 0.0;     // the staging and reduction of the last bh_step call (profiling)
    int64_t slog_launches = 0;

    // bh_render_bodies (render.hip): buffers of its own, allocated on first use, kept while the
    // padded pixel count is unchanged.  rnd_packed / rnd_cnt are zero between calls (the resolve
    // kernel re-zeroes what the rasteriser touched); rnd_clean = false: a call failed in between
    uint32_t *rnd_packed = nullptr, *rnd_cnt = nullptr;
    uint8_t *rnd_pixels = nullptr;                        // staged planes, device
    uint32_t *rnd_owner = nullptr, *rnd_counts = nullptr;
    size_t rnd_pad = 0;  // padded pixels the buffers above are sized for
    uint8_t *rnd_pin = nullptr;  // pinned host bounce buffer of the staged planes
    size_t rnd_pin_bytes = 0;
    bool rnd_clean = false;
    Stopwatch rnd_sw;  // around the last render's two kernels

    // bh_render_quads (render_quads.hip): buffers of its own, allocated on first use, kept while
    // the pixel count is unchanged.  The three working planes are zero between calls (the scans
    // re-zero what the cell kernel touched); qd_clean = false: a call failed in between
    uint32_t *qd_rowd = nullptr, *qd_cold = nullptr, *qd_dir = nullptr;
    uint32_t *qd_out = nullptr;               // the staged count plane, device
    unsigned long long *qd_count = nullptr;   // the cell count in partial sums, device
    size_t qd_pix = 0;  // pixels the planes above are sized for
    bool qd_clean = false;
    Stopwatch qd_sw;  // around the last call's kernels

    bool tree_valid = false;  // lastTree (BHA:304): keys_s / cpl / base / nodes are current
    // Multi-rank engines end a call with a LET build too; lastTree is then built on demand by
    // bh_get_quads from the positions that build saw (lt_x, lt_y), without touching the state
    bool lazy_tree = false;
    double *lt_x = nullptr, *lt_y = nullptr;
    int64_t lt_cap = 0;

    // Hilbert lane map of the single-GPU traversal (tree_build.hip lane_order): lane -> slot
    uint32_t *lanes = nullptr;
    bool lanes_valid = false;  // the map is a permutation of the current slots
    int lanes_age = 0;         // builds since the last Hilbert sort
    bool lane_sort = false;    // BH_LANE_ORDER_SORT=1 at creation: re-sort with the radix sort
    // a due re-sort of the pipelined step's lane map, run beside the next first traversal on its
    // own buffers (lane_refresh_beside) and swapped in before the second build
    bool lr_pending = false;   // a re-sort is due from the prebuilt tree's keys
    bool lr_ready = false;     // lanes_next holds it once lr_ev completes
    uint32_t *lanes_next = nullptr, *lr_hkey = nullptr, *lr_hkey_s = nullptr, *lr_slot = nullptr;
    void *lr_scratch = nullptr;
    size_t lr_scratch_bytes = 0;
    int64_t lr_cap = 0;
    hipEvent_t lr_ev = nullptr;
    const uint32_t *a2_lanes = nullptr;  // the last evaluation wrote a2 by lane of this map
    GatherLayout a2_layout{};            // ... at the lane's gather slot (multi-rank rounds)

    // multi-rank locally essential tree (let.hip): subset state and tree workspace
    // BH_LET unset: LET builds from BH_LET_MIN_WORLD ranks up (round 3, solo C4 rank 0, ms per
    // step LET / replicated: 2 ranks 9.80 / 10.21, 3 ranks 7.00 / 7.98, 4 ranks 5.53 / 6.80,
    // 8 ranks 3.43 / 5.19; round 2 had 10.45 / 10.15 at 2 ranks, hence 4 then);
    // BH_LET=1 at any world size, BH_LET=0 never
    bool let_on = true;
    bool let_forced = false;
    int let_age = 0;            // LET builds since the last full build
    int64_t let_builds = 0, full_builds = 0, let_last_sub = 0;
    int64_t let_known = 0;       // largest subset of the last bh_step call (0: unknown)
    int64_t let_overflows = 0;   // calls replayed for a subset overflow
    uint32_t s_spl_nb = 0;       // splitters of the last LET build (subset bucket sort)
    bool st_morton = false;     // slots are in the Morton order of a full build (not caller order)
    bool vel_stale = false;     // LET evaluations integrated only own bodies: velocities of the
                                // others are exchanged before the next full build
    LetBufs L{};
    int64_t let_cap = 0;        // n capacity of the per-body LET arrays
    // the selection's candidate blocks (let.hip LetSweep): the boxes of the state's 256-slot
    // blocks at the last full build, and the displacement bound since (disp[0]; the speed words
    // after it: own, then every rank's, exchanged at the end of every drifting LET evaluation)
    uint32_t *let_box = nullptr;
    double *disp = nullptr;
    bool boxes_valid = false;
    // the selection's marks were cleared by the last LET build's lane map (for n bodies)
    bool let_clean = false;
    int64_t let_clean_n = -1;
    int builds_since_box = 0;   // builds since then that may have jittered positions
    int64_t let_sub_cap = 0;    // subset capacity of the subset tree workspace
    int let_J = -1;
    size_t let_node_cap = 0;
    BodyState sub_src{}, sub_dst{};
    uint64_t *s_keys = nullptr, *s_keys_s = nullptr, *s_spl = nullptr;
    uint32_t *s_keys32 = nullptr, *s_keys32_s = nullptr, *s_idx = nullptr, *s_perm = nullptr;
    int8_t *s_cpl = nullptr;
    uint32_t *s_cnt = nullptr, *s_base = nullptr, *s_cell_start = nullptr;
    uint32_t *s_span_list = nullptr, *s_super_list = nullptr, *s_bcount = nullptr,
             *s_bstart = nullptr;
    bh::SpanSlot *s_span_children = nullptr;
    Node *s_nodes = nullptr;
    hipEvent_t table_ev = nullptr;
    int64_t set_cap = 0;        // n capacity of the per-body arrays L.lanes, L.subpos
    hipEvent_t sub_cnt_ev = nullptr;
    uint32_t *sub_cnt_h = nullptr;    // pinned: the last selection's subset size (sub_cnt_ev)
    bool sub_cnt_pending = false;

    LetCell *pub_table = nullptr;     // in-process group: the table this member exchanges now
    hipEvent_t pub_table_ev = nullptr;
    bool inject_guard = false;  // bh_debug_inject(1): the next LET build trips k_let_guard
    int inject_build = -1;      // bh_debug_inject(2 + k): the k-th next full build raises its
                                // jitter flag (as the unsupported-geometry guard would)
    bool agree_failed = false;  // in-process group: this member could not read a peer's flags
    // pipelined step (one GPU): the next step's first build runs on pipe_stream while this step's
    // second traversal runs; it builds into nodes_alt / alt, and the traversal reads copies of
    // what that build and the merge rule overwrite (masses, flags, lane map, node count)
    Node *nodes_alt = nullptr;
    size_t nodes_alt_cap = 0;
    double *m_trav = nullptr;
    uint32_t *cidx_trav = nullptr, *lanes_trav = nullptr, *T_trav = nullptr;
    int64_t trav_cap = 0;
    bool prebuilt = false;  // the current step's first build was made by the previous step
    // ... by the previous call's last step: that build's error flags are in scalars[10] (they
    // belong to the step that uses the tree, the next call's first, which takes them over)
    bool carried_flags = false;
    // the velocities are still in the previous slot order, in alt (the overlapped build's
    // permutation, read by the next step's first kick); null: st holds them
    const uint32_t *vel_perm = nullptr;
    bool fuse_keys = false;   // the next KICK_DRIFT traversal writes the next build's keys / buckets
    bool keys_ready = false;  // ... and it did: the next full build skips k_morton, k_bucket_count
    hipEvent_t pipe_ev[3] = {nullptr, nullptr, nullptr};
    hipStream_t pipe_stream = nullptr;  // the overlapped work's stream (the highest priority)
    // A call's last step is pipelined too (the front-end calls bh_step(1) once per frame): the
    // call then ends with the next step's first tree already built (prebuilt: st in its order,
    // jitter applied, nodes).  What the caller sees -- the reference's bodies after step(), before
    // the next buildTree's jitter (BHA:146-151) -- is `view` (the previous slot order); lastTree
    // (BHA:435) is nodes_alt with its walk structures copied aside (lt_keys, lt_cpl, lt_base).
    // The next bh_step consumes the prebuilt tree; bh_set_params (geometry), bh_reset_bodies and
    // a replay drop it.
    BodyState view{};
    int64_t view_cap = 0;
    bool view_pending = false;
    uint64_t *lt_keys = nullptr;
    int8_t *lt_cpl = nullptr;
    uint32_t *lt_base = nullptr;
    int64_t lt_walk_cap = 0;
    bool lt_aside = false;  // lastTree is (nodes_alt, lt_keys, lt_cpl, lt_base)
    // Pinned caller-order mirror of the bodies (bh_set_mirror / bh_map_bodies): x, y, vx, vy, m
    // at stride mir_cap, filled by the step itself on mir_stream
    bool mirror_on = false;
    double *mir = nullptr;        // pinned host, 5 * mir_cap: the buffer the copies write
    // bh_set_mirror(e, 2): two buffers; the copies write the one bh_map_bodies did not hand out
    // last (mir_front), so a caller reads the mapped bodies while the next bh_step runs
    double *mir_buf[2] = {nullptr, nullptr};
    int mir_nbuf = 1;
    int mir_front = -1;
    double *mir_stage = nullptr;  // device, 5 * mir_cap (caller order, compacted)
    uint32_t *mir_keep = nullptr, *mir_pos = nullptr;  // device, caller order
    int64_t mir_cap = 0;
    void *mir_tmp = nullptr;      // the mirror's scan scratch (the overlapped build uses `scratch`)
    size_t mir_tmp_bytes = 0;
    bool mir_fresh = false;       // the mirror (after mir_ev) holds the current caller state
    bool mir_launched = false;    // ... launched by the running call's last step
    int64_t mir_n = 0;
    hipStream_t mir_stream = nullptr;
    hipEvent_t mir_ev = nullptr;   // copy-out complete
    hipEvent_t mir_ev2 = nullptr;  // the mirror's kernels are done reading the state
    hipEvent_t mir_in[2] = {nullptr, nullptr};
    // bh_step_begin / bh_step_positions / bh_step_end (two mirror buffers only): the call runs
    // on step_thr of the handle the caller holds; the engine that fills the mirror (this one, or
    // a multi handle's member 0) hands over positions, masses and the survivors' list indices of
    // the running call once its last merge rule is done (mid_*), before the last traversal
    std::thread step_thr;
    std::atomic<bool> async_running{false};
    int async_rc = 0;
    int64_t mid_n0 = 0;              // bodies before the running call
    bool mid_surv_done = false;      // the survivors were derived from the call's removals
    bh_engine *mid_eng = nullptr;    // the running call's mirror engine
    std::mutex mid_mu;
    std::condition_variable mid_cv;
    bool mid_armed = false, mid_ready = false, mid_done = false, mid_void = false;
    double *mid_buf = nullptr;       // the mirror buffer of the hand-off
    int64_t mid_stride = 0;
    hipEvent_t mid_ev = nullptr;     // the hand-off's copies are done
    hipEvent_t mid_sv_ev = nullptr;  // ... its survivors' (copied first)
    // pinned, MIRROR_HDR + mir_cap (mirror_survivors): scalars[0..4) at the hand-off (tree
    // flags, removals, mailbox overflow), then survivor j's index in the list before the call
    uint32_t *mir_idx = nullptr;
    uint32_t *mir_idx_stage = nullptr;  // device, the same
    hipEvent_t mir_ev3 = nullptr;
    // one GPU: the previous evaluation's wave durations and the longest-first run order
    // (slot 0: the one-GPU launch over all lanes; 1 + k: LET round k's piece)
    uint32_t *wave_cost = nullptr, *run_order = nullptr;
    int64_t cost_stride = 0, order_stride = 0;
    int64_t order_n[1 + BH_SHARD_ROUNDS] = {};  // run_order slot j: a permutation of the runs
                                               // of a launch over order_n[j] lanes (0: none)
    // Between LET evaluations the new positions stay in the exchange buffer (a2, by lane of
    // pos_lanes at pos_layout's gather slots): the next selection reads them there, and the
    // replica's x, y are written only when something else needs them (materialize_positions)
    bool pos_pending = false;
    const uint32_t *pos_lanes = nullptr;
    GatherLayout pos_layout{};
    uint32_t *inv_lanes = nullptr;  // slot -> gather slot of its lane (the selection's reads)
    bool inv_valid = false;         // ... for the current lane map, n and layout
    // bh_create_solo (measurement): no peers; their cells' values from the last full build
    bool solo = false;
    LetCell *solo_table = nullptr;
    uint8_t *solo_all = nullptr;    // every cell marked
    double *solo_xchg = nullptr;    // BH_SOLO_XCHG: receive buffer of the emulated exchange
    int64_t solo_xchg_cap = 0;
    uint32_t *solo_cstart = nullptr;

    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_phase;
    size_t ev_used = 0;
    double phase_ms[kPhases] = {0, 0, 0, 0, 0};
    double trav_ms_sum = 0.0;
    int64_t trav_launches = 0;
    std::vector<double> trav_samples;  // per-launch traversal times of the last call (ms)
    bool timings_pending = false;

    // the collectives this rank issued, in host issue order (bh_collective_log): every rank of a
    // decomposition must issue the same sequence, or RCCL pairs mismatched calls and hangs
    std::vector<int64_t> coll_log;  // (api call, site, bytes, stream) per collective
    int64_t api_calls = 0;          // state-changing API calls made on this engine

    // Failure of a multi-rank call (the reference's join always returns, BHA:408, 426): a rank
    // whose call fails -- or that finds a peer failed, or waits past BH_COMM_TIMEOUT_S -- marks
    // itself failed, aborts its in-process group / RCCL communicator (ncclCommAbort) so that no
    // peer waits for it, and every state-changing call returns BH_E_COMM until bh_reset_bodies
    std::atomic<bool> *abort_flag = nullptr;  // a multi-device handle's members: shared, set by
                                              // any member that failed (multi.cpp)
    bool comm_failed = false;
    bool comm_lost = false;      // the RCCL communicator was aborted (a new one is needed)
    std::string fail_msg;
    int inject_coll = -1;        // bh_debug_inject(100 + k): fail before the k-th next collective
    int inject_barrier = -1;     // bh_debug_inject(200 + k): ... before the k-th next group barrier
    // progress, readable from any thread while a call runs (bh_progress: heartbeats)
    std::atomic<int64_t> prog_api{0}, prog_coll{0};
    std::atomic<int> prog_site{0}, prog_busy{0};

    std::string err;

    // bh_compute_radial_profile (radial_profile.hip): the call's own buffers, allocated on first
    // use and grown when the list outgrows them (rad_cap bodies; the planes that depend on the bin
    // count are sized for BH_RADIAL_MAX_BINS) or the subset does (rad_sub_cap entries)
    uint32_t *rad_u32 = nullptr;   // key, sorted key, index, sorted index; the keys' starts
    uint8_t *rad_flag = nullptr;   // the subset's marks, by caller index
    double *rad_f64 = nullptr;     // the seven term planes; the blocks' partial sums; the edges
    bh_radial_bin *rad_bins = nullptr;
    int64_t *rad_sub = nullptr;    // the uploaded subset
    void *rad_scratch = nullptr;   // the sort
    size_t rad_scratch_bytes = 0;
    int64_t rad_cap = 0, rad_sub_cap = 0;
    Stopwatch rad_sw;  // from the staging in list order to the last emit kernel
};

namespace {

#define HIPCHK(e, expr)                                                                  \
    do {                                                                                 \
        hipError_t _st = (expr);                                                         \
        if (_st != hipSuccess) {                                                         \
            (e)->err = std::string(#expr) + ": " + hipGetErrorString(_st);              \
            return BH_E_DEVICE;                                                          \
        }                                                                                \
    } while (0)

#define NCCLCHK(e, expr)                                                                 \
    do {                                                                                 \
        ncclResult_t _st = (expr);                                                       \
        if (_st != ncclSuccess) {                                                        \
            (e)->err = std::string(#expr) + ": " + ncclGetErrorString(_st);              \
            return BH_E_COMM;                                                            \
        }                                                                                \
    } while (0)

#define TRY(expr)                      \
    do {                               \
        int _rc = (expr);              \
        if (_rc != BH_OK) return _rc;  \
    } while (0)

// One collective of a multi-rank engine (RCCL call, or its in-process copies): logged so that
// tests can check that every rank issues the same sequence (bh_collective_log).
enum CollSite {
    COLL_ACC = 1,       // a round of accelerations (full evaluation), in-place all-gather
    COLL_POS = 2,       // a round of new positions (LET evaluation)
    COLL_VEL = 3,       // a round of owners' velocities (before a full build, at a call's end)
    COLL_TABLE = 4,     // the LET cell tables
    COLL_FLAGS = 5,     // the end-of-call LET status words, max all-reduce
    COLL_SETTINGS = 6,  // the per-process settings check at creation (min and max all-reduce)
    COLL_VMAX = 7,      // every rank's drift speed bound (LET selection), after a drifting round
};
enum CollStream { CS_MAIN = 0, CS_COMM = 1 };
// Called before every collective: logs it, counts it for the heartbeat, and trips an injected
// host-side failure (bh_debug_inject(100 + k)) -- the rank then returns before the collective its
// peers have issued, exactly as a rank-local error would.
int coll_log(bh_engine *e, int site, int64_t bytes, int stream) {
    if (e->world <= 1 && !e->comm) return BH_OK;
    if (e->inject_coll >= 0 && e->inject_coll-- == 0) {
        e->err = "injected host-side failure before a collective (bh_debug_inject)";
        return BH_E_COMM;
    }
    e->prog_coll.fetch_add(1);
    e->prog_site.store(site);
    if (e->coll_log.size() >= ((size_t)1 << 22)) return BH_OK;  // (bounded: 1 M entries)
    e->coll_log.insert(e->coll_log.end(), {e->api_calls, (int64_t)site, bytes, (int64_t)stream});
    return BH_OK;
}

bool multi_rank(const bh_engine *e) { return (e->comm || e->group || e->comm_lost) && !e->solo; }

bool peers_aborted(const bh_engine *e) {
    return (e->group && e->group->aborted.load()) || (e->abort_flag && e->abort_flag->load());
}

// An in-process group's barrier, with its way out: false from an aborted group -> BH_E_COMM.
int group_barrier(bh_engine *e) {
    if (e->inject_barrier >= 0 && e->inject_barrier-- == 0) {
        e->err = "injected host-side failure before a group barrier (bh_debug_inject)";
        return BH_E_COMM;
    }
    if (!e->group->barrier()) {
        std::lock_guard<std::mutex> lk(e->group->mu);
        e->err = e->group->timed_out
                     ? "group barrier: a peer did not arrive within BH_COMM_TIMEOUT_S"
                     : "group barrier: aborted (a peer rank's call failed)";
        return BH_E_COMM;
    }
    return BH_OK;
}

// Poll stream s until it is idle, at most `secs` seconds (0: forever).  hipErrorNotReady on expiry.
hipError_t drain_stream(hipStream_t s, double secs) {
    if (!s) return hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0;; ++spins) {
        const hipError_t q = hipStreamQuery(s);
        if (q != hipErrorNotReady) return q;
        if (secs > 0.0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > secs)
            return hipErrorNotReady;
        if (spins < 2000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// Abort this rank's RCCL communicator (its kernels waiting for peers exit) and let every stream
// of the engine drain, bounded.  The engine keeps no communicator afterwards (comm_lost).
void abort_comm(bh_engine *e) {
    if (e->comm) {
        (void)ncclCommAbort(e->comm);
        e->comm = nullptr;
        e->comm_lost = true;
    }
    for (hipStream_t s : {e->stream, e->stream2, e->comm_stream, e->pipe_stream, e->mir_stream})
        (void)drain_stream(s, 30.0);
}

// A multi-rank call failed on this rank (rc != BH_OK): mark the engine failed and make sure no
// peer waits for it -- abort the in-process group or the multi-device handle's members (the
// flag every member's waits poll), and this rank's communicator.
int fail_multi_rank(bh_engine *e, int rc) {
    if (rc == BH_OK || !multi_rank(e)) return rc;
    if (!e->comm_failed) e->fail_msg = e->err;
    e->comm_failed = true;
    if (e->group) e->group->abort();
    if (e->abort_flag) e->abort_flag->store(true);
    abort_comm(e);
    return rc;
}

// Wait until stream s is idle.  Multi-rank engines poll: a collective whose peers never arrive
// would block a plain hipStreamSynchronize forever.  With RCCL the wait ends -- the communicator
// aborted, BH_E_COMM -- on an asynchronous RCCL error, when another member of the handle failed,
// or after BH_COMM_TIMEOUT_S; an in-process group's device waits are on recorded events and
// always end (its barriers carry the abort), so it only gets the deadline.
int wait_stream(bh_engine *e, hipStream_t s) {
    if (!multi_rank(e)) {
        HIPCHK(e, hipStreamSynchronize(s));
        return BH_OK;
    }
    const double limit = comm_timeout_s();
    const auto t0 = std::chrono::steady_clock::now();
    const char *why = nullptr;
    for (int spins = 0;; ++spins) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) return BH_OK;
        if (q != hipErrorNotReady) {
            e->err = std::string("hipStreamQuery: ") + hipGetErrorString(q);
            return BH_E_DEVICE;
        }
        if (e->comm) {
            ncclResult_t ar = ncclSuccess;
            if (ncclCommGetAsyncError(e->comm, &ar) == ncclSuccess && ar != ncclSuccess &&
                ar != ncclInProgress)
                why = "RCCL reported an asynchronous error";
            else if (e->abort_flag && e->abort_flag->load())
                why = "another member of the handle failed";
        }
        if (!why && limit > 0.0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit)
            why = "timed out (BH_COMM_TIMEOUT_S) waiting for the device: a collective whose peers "
                  "never arrived?";
        if (why) break;
        if (spins < 2000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    e->err = std::string("wait for the device: ") + why;
    abort_comm(e);
    return BH_E_COMM;
}

#define SYNC(e, s) TRY(wait_stream((e), (s)))

// Root cell (BHA:360-361) and the exact per-depth half-sizes (BHA:74).
int make_geometry(const bh_params &p, Geometry &g, std::string &err) {
    if (p.width_px <= 0 || p.height_px <= 0) {
        err = "width_px and height_px must be positive";
        return BH_E_INVALID;
    }
    std::memset(&g, 0, sizeof(g));
    const int W = p.width_px, H = p.height_px;
    g.root_cx = (double)W / 2.0;
    g.root_cy = (double)H / 2.0;
    g.root_h = (double)std::max(W, H) / 2.0 + 2.0;
    g.h[0] = g.root_h;
    for (int d = 1; d < MAX_DEPTH_TAB; ++d) g.h[d] = g.h[d - 1] / 2.0;
    int J = -1;
    for (int d = 0; d < MAX_DEPTH_TAB; ++d)
        if (g.h[d] < 1e-3) {
            J = d;
            break;
        }
    if (J < 1 || J > 30 || J + 3 > MAX_DEPTH_TAB) {
        err = "root cell too large for 64-bit Morton keys (jitter depth > 30)";
        return BH_E_INVALID;
    }
    g.J = J;
    for (int d = 0; d < MAX_DEPTH_TAB; ++d) {
        double s = g.h[d] * 2.0;  // BHA:226
        g.s2[d] = s * s;
    }
    return BH_OK;
}

template <typename T>
int dev_alloc(bh_engine *e, T *&ptr, size_t count) {
    if (ptr) {
        (void)hipFree(ptr);
        ptr = nullptr;
    }
    if (count == 0) count = 1;
    HIPCHK(e, hipMalloc((void **)&ptr, count * sizeof(T)));
    return BH_OK;
}

// Grow-or-keep of buffers that share the capacity `cap`: false while `need` entries fit and the
// buffers (`first`: one of them) exist.  Else the caller allocates them anew and then sets cap;
// cap is 0 meanwhile, so after a failed allocation the next call allocates again.
bool outgrown(int64_t &cap, const void *first, int64_t need) {
    if (need <= cap && first) return false;
    cap = 0;
    return true;
}

}  // namespace

int Stopwatch::start(bh_engine *e, hipStream_t s) {
    for (hipEvent_t &v : ev)
        if (!v) HIPCHK(e, hipEventCreate(&v));
    HIPCHK(e, hipEventRecord(ev[0], s));
    return BH_OK;
}

int Stopwatch::stop(bh_engine *e, hipStream_t s) {
    HIPCHK(e, hipEventRecord(ev[1], s));
    timed = true;
    return BH_OK;
}

int Stopwatch::ms(double *out) const {
    *out = 0.0;
    if (!timed) return BH_OK;
    float f = 0.f;
    if (hipEventElapsedTime(&f, ev[0], ev[1]) != hipSuccess) return BH_E_DEVICE;
    *out = (double)f;
    return BH_OK;
}

void Stopwatch::destroy() {
    for (hipEvent_t &v : ev) {
        if (v) (void)hipEventDestroy(v);
        v = nullptr;
    }
    timed = false;
}

namespace {

int alloc_state(bh_engine *e, BodyState &s, size_t cap) {
    TRY(dev_alloc(e, s.x, cap));
    TRY(dev_alloc(e, s.y, cap));
    TRY(dev_alloc(e, s.vx, cap));
    TRY(dev_alloc(e, s.vy, cap));
    TRY(dev_alloc(e, s.m, cap));
    TRY(dev_alloc(e, s.cidx, cap));
    return BH_OK;
}

size_t node_capacity(int64_t n, int J) {
    // T = sum_a (1 + max(0, c(a) - c(a-1))) <= n + (J+1) * (n/2 + 2)
    return (size_t)n + (size_t)(J + 1) * ((size_t)n / 2 + 2) + 16;
}

// Capacity for n bodies.  Growing drops the live state (callers reset it); a change of the
// jitter depth J only re-sizes the tree workspace.
int ensure_capacity(bh_engine *e, int64_t n) {
    const int J = e->geo.J;
    if (n <= e->cap && J == e->J_alloc) return BH_OK;
    const int64_t cap = std::max<int64_t>(n, std::max<int64_t>(e->cap, 1));
    if (n > e->cap || !e->st.x) {
        TRY(alloc_state(e, e->st, cap));
        TRY(alloc_state(e, e->alt, cap));
        // multi-GPU: rounds x world pieces of whole wavefronts (bh_shard_range)
        const int64_t padded = (e->comm || e->group || e->solo) ? shard_sub(cap, e->world, BH_SHARD_ROUNDS) *
                                             e->world * BH_SHARD_ROUNDS
                                       : cap;
        TRY(dev_alloc(e, e->a2, 2 * padded));
        TRY(dev_alloc(e, e->ax, cap));
        TRY(dev_alloc(e, e->ay, cap));
        TRY(dev_alloc(e, e->keys, cap));
        TRY(dev_alloc(e, e->keys_s, cap));
        TRY(dev_alloc(e, e->keys32, cap));
        TRY(dev_alloc(e, e->keys32_s, cap));
        TRY(dev_alloc(e, e->idx, cap));
        TRY(dev_alloc(e, e->perm, cap));
        TRY(dev_alloc(e, e->perm2, cap));
        TRY(dev_alloc(e, e->cpl, cap + 32));  // slack for word-wise scans
        TRY(dev_alloc(e, e->cnt, cap + 1));
        TRY(dev_alloc(e, e->base, cap + 1));
        TRY(dev_alloc(e, e->visits32, cap));
        TRY(dev_alloc(e, e->contrib32, cap));
        TRY(dev_alloc(e, e->lanes, cap));
        e->lanes_valid = e->lr_pending = e->lr_ready = false;
        e->inv_valid = false;
        TRY(dev_alloc(e, e->wave_iters, cap / 64 + 2));
        TRY(dev_alloc(e, e->wave_blocks, cap / 64 + 2));
        e->cost_stride = cap / 64 + 2;
        e->order_stride = (int64_t)wave_order_runs(cap) + 1;
        TRY(dev_alloc(e, e->wave_cost, (size_t)(e->cost_stride * (1 + BH_SHARD_ROUNDS))));
        HIPCHK(e, hipMemsetAsync(e->wave_cost, 0,
                                 sizeof(uint32_t) * (size_t)(e->cost_stride * (1 + BH_SHARD_ROUNDS)),
                                 e->stream));
        TRY(dev_alloc(e, e->run_order, (size_t)(e->order_stride * (1 + BH_SHARD_ROUNDS))));
        for (int64_t &o : e->order_n) o = 0;
        TRY(dev_alloc(e, e->heavy, cap));
        TRY(dev_alloc(e, e->keep, cap));
        TRY(dev_alloc(e, e->pos, cap));
        TRY(dev_alloc(e, e->spl, (size_t)sort_buckets(cap) + 2));
        TRY(dev_alloc(e, e->bcount, (size_t)sort_buckets(cap) + 2));
        TRY(dev_alloc(e, e->bstart, (size_t)sort_buckets(cap) + 2));
        HIPCHK(e, hipMemsetAsync(e->bcount, 0, sizeof(uint32_t) * ((size_t)sort_buckets(cap) + 2),
                                 e->stream));
        e->spl_nb = 0;
        e->keys_ready = false;
        e->cap = cap;
    }
    size_t ncap = node_capacity(e->cap, J);
    if (ncap > e->node_cap || J != e->J_alloc) {
        TRY(dev_alloc(e, e->nodes, ncap));
        TRY(dev_alloc(e, e->span_list, (size_t)(J + 2) * span_stride_for(e->cap)));
        TRY(dev_alloc(e, e->span_children, (size_t)(J + 2) * span_stride_for(e->cap)));
        TRY(dev_alloc(e, e->super_list,
                      (size_t)(J + 2) * span_groups(span_stride_for(e->cap))));
        TRY(dev_alloc(e, e->cell_start,
                      ((size_t)1 << (2 * std::min(J, CELL_TABLE_MAX_DEPTH))) + 2));
        e->node_cap = ncap;
        e->J_alloc = J;
    }
    size_t cb = std::max(tree_scratch_bytes(e->cap, J), compact_scratch_bytes(e->cap));
    cb = std::max(cb, let_scratch_bytes(e->cap));
    if (cb > e->scratch_bytes) {
        if (e->scratch) (void)hipFree(e->scratch);
        e->scratch = nullptr;
        HIPCHK(e, hipMalloc(&e->scratch, cb));
        e->scratch_bytes = cb;
    }
    return BH_OK;
}

TreeBuffers tree_buffers(bh_engine *e) {
    TreeBuffers b;
    b.src = e->st;
    b.dst = e->alt;
    b.keys = e->keys;
    b.keys_s = e->keys_s;
    b.keys32 = e->keys32;
    b.keys32_s = e->keys32_s;
    b.idx = e->idx;
    b.perm = e->perm;
    b.cpl = e->cpl;
    b.cnt = e->cnt;
    b.base = e->base;
    b.cell_start = e->cell_start;
    b.nodes = e->nodes;
    b.scalars = e->scalars;
    b.span_list = e->span_list;
    b.span_stride = span_stride_for(e->cap);
    b.span_children = e->span_children;
    b.super_list = e->super_list;
    b.scratch = e->scratch;
    b.scratch_bytes = e->scratch_bytes;
    b.spl = e->spl;
    b.spl_nb = e->spl_nb;
    b.bcount = e->bcount;
    b.bstart = e->bstart;
    b.lane_sort = e->lane_sort;
    return b;
}

// ---- profiling events ----------------------------------------------------------------
constexpr int PHASE_START = -2;         // mark(): a start marker even right behind another mark
constexpr int PHASE_TRACERS = kPhases;  // mark(): the interval was a tracer walk (phase [1])
constexpr int PHASE_STEP_LOG = kPhases + 1;  // ... the step log's staging and reduction (phase [2])
int mark(bh_engine *e, int phase) {  // close the interval of `phase` begun at the last mark
    if (!e->profiling) return BH_OK;
    // phases are contiguous on the stream: the previous phase's end mark starts the next one
    // (PHASE_START: a start marker of its own, for an interval that excludes what was queued
    // since the last mark)
    if (phase == -1 && e->ev_used > 0) return BH_OK;
    if (e->ev_used + 1 > e->ev.size()) {
        // timing-only events: a device-scope release, no system-scope fence (the default one
        // writes back and invalidates the caches: ~10 us of idle GPU per event in the step)
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableSystemFence) != hipSuccess) {
            (void)hipGetLastError();
            HIPCHK(e, hipEventCreate(&ev));
        }
        e->ev.push_back(ev);
        e->ev_phase.push_back(-1);
    }
    HIPCHK(e, hipEventRecord(e->ev[e->ev_used], e->stream));
    e->ev_phase[e->ev_used] = phase;  // phase of the interval ending here (-1: start marker)
    ++e->ev_used;
    e->timings_pending = true;
    return BH_OK;
}

int collect_timings(bh_engine *e) {
    if (!e->timings_pending) return BH_OK;
    SYNC(e, e->stream);
    for (int k = 0; k < kPhases; ++k) e->phase_ms[k] = 0.0;
    e->trav_ms_sum = 0.0;
    e->trav_launches = 0;
    e->trav_samples.clear();
    e->trc_ms_sum = 0.0;
    e->trc_launches = 0;
    e->slog_ms_sum = 0.0;
    e->slog_launches = 0;
    for (size_t i = 1; i < e->ev_used; ++i) {
        int ph = e->ev_phase[i];
        if (ph < 0) continue;
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, e->ev[i - 1], e->ev[i]));
        if (ph == PHASE_TRACERS) {  // a tracer walk: under the traversal's phase, counted apart
            e->phase_ms[1] += ms;
            e->trc_ms_sum += ms;
            ++e->trc_launches;
            continue;
        }
        if (ph == PHASE_STEP_LOG) {  // a step's record: under the integration's phase
            e->phase_ms[2] += ms;
            e->slog_ms_sum += ms;
            ++e->slog_launches;
            continue;
        }
        e->phase_ms[ph] += ms;
        if (ph == 1) {  // per evaluation
            e->trav_ms_sum += ms;
            ++e->trav_launches;
            e->trav_samples.push_back(ms);
        }
    }
    e->timings_pending = false;
    return BH_OK;
}

// ---- buildTree() (BHA:359-366): sort + build; the state moves to the new Morton order ----
#ifndef BH_LANE_REFRESH
// builds between Hilbert re-sorts of the lane map (0: Morton lanes).  With the re-sort beside the
// first traversal (lane_refresh_beside) a fresher map pays: C3 1.84-1.85 ms per step at 16, 1.82-1.83 at
// 8, 1.814-1.820 at 6, 1.82-1.83 at 4 (round 4, profiles/r04L2_lane_refresh_ab.txt) -- with the
// radix sort, ~0.76 ms of kernels per re-sort.  The run scatter (tree_build.hip lane_order_into)
// takes ~0.06 ms beside the traversal: means of 6 interleaved runs 1.7122 at 6, 1.7079 at 3,
// 1.7081 at 2, 1.7129 at 1, the sort at 6 1.7151 (profiles/r07_lane_scatter_ab.md: all within
// each other's spread)
#define BH_LANE_REFRESH 3
#endif
#ifndef BH_LANE_REFRESH_SHARDED
#define BH_LANE_REFRESH_SHARDED 16  // multi-rank engines (no pipelined step: the re-sort is in line)
#endif
// "theta is zero" is a statement about theta^2, the value the criterion uses (BHA:226-228) and
// the one evaluate() picks the all-pairs kernel by: for 0 < |theta| < ~1.5e-162 the square
// underflows to zero.  Everything that prepares for a tree walk (lane maps, pipelining, LET
// builds, the snapshot) asks this, so that it never disagrees with the kernel choice.
bool theta2_is_zero(const bh_engine *e) { return e->p.theta * e->p.theta == 0.0; }

// The force-evaluation constants (BHA:378) of the engine's parameters, with the root's opening
// threshold for its geometry (open_threshold.hpp): the one place every evaluation gets them.
ForceParams force_params(const bh_engine *e) {
    const double theta2 = e->p.theta * e->p.theta;
    return ForceParams{e->p.G, e->p.soft2, theta2, open_threshold(e->geo.s2[0], theta2)};
}

// What one build is asked for (build_into), and what it did.
struct BuildRequest {
    // the pipelined step's next tree, built on stream `s` beside the second traversal into
    // nodes_alt / alt with its own permutation (perm2; the traversal reads perm), velocities left
    // to permute_velocities, and without the final swap (the caller swaps)
    bool overlap;
    // the velocities stay in the previous slot order (in alt after the swap) for a traversal that
    // permutes them as it kicks (KickArgs::perm)
    bool keep_v;
    // a call's last overlapped build, whose tree the next call uses -- its error flags go to
    // scalars[10] instead of the running call's scalars[1] (evaluate / bh_get_quads take them over)
    bool carry;
    // k_prep lists the merge rule's heavy bodies in this build's order (the rule follows the
    // build before any other build: masses change only in the rule, BHA:518)
    bool heavy_list;
    // a due re-sort of the lane map is left to lane_refresh_beside: by the second build
    // (lane_hold, to the next overlapped one) and by an overlapped build that may (lane_defer)
    bool lane_hold, lane_defer;
    // the second traversal's input copies (m_trav ...) made by k_emit_com, which also clears the
    // merge rule's mailbox header tc_box
    bool tc_want;
    uint32_t *tc_box;
    // the overlapped chain's fork inside the second build (TreeBuffers::fork_ev / late_ev): the
    // event a build that makes the copies records after its k_emit_com, and the one an overlapped
    // build waits for before it writes the span lists
    hipEvent_t fork_want, chain_late;
    // out: the build made the copies; it recorded fork_want
    bool tc_done, forked;
};

int build_into(bh_engine *e, hipStream_t s, BuildRequest &rq) {
    const bool overlap = rq.overlap;
    const int64_t n = e->n;
    TreeBuffers tb = tree_buffers(e);
    if (rq.heavy_list && e->heavy_dirty)  // (a list no rule consumed: a call that failed between)
        HIPCHK(e, hipMemsetAsync(e->scalars + 14, 0, sizeof(uint32_t), s));
    e->heavy_ready = rq.heavy_list && n > 0;
    if (e->heavy_ready) {
        e->heavy_dirty = true;
        tb.heavy = e->heavy;
        tb.heavy_count = e->scalars + 14;
        tb.heavy_thr = e->p.merge_max_mass;
    }
    if (overlap) {
        tb.src.vx = tb.src.vy = nullptr;
        tb.nodes = e->nodes_alt;
        tb.perm = e->perm2;
    }
    if (rq.carry) tb.scalars = e->scalars + 9;  // (the build writes scalars[1] of its buffers)
    if (rq.keep_v) tb.src.vx = tb.src.vy = nullptr;
    // Hilbert waves (every rank alike): re-sorted every BH_LANE_REFRESH builds, carried through
    // the build's permutation by k_emit_com in between
    const bool use_lanes = BH_LANE_REFRESH > 0 && n > 0 && !theta2_is_zero(e);
    const int every = (e->comm || e->group || e->solo) ? BH_LANE_REFRESH_SHARDED : BH_LANE_REFRESH;
    const bool due = use_lanes && e->lanes_valid && e->lanes_age >= every;
    // (pipelined steps: the re-sort is left to the next first traversal's side, see
    // lane_refresh_beside; the map is carried through this build meanwhile)
    const bool defer = due && ((overlap && rq.lane_defer) || rq.lane_hold);
    const bool refresh = use_lanes && (!e->lanes_valid || (due && !defer));
    tb.lanes_remap = use_lanes && !refresh ? e->lanes : nullptr;
    // the second traversal's copies made by the build (k_emit_com) instead of k_trav_inputs --
    // not when the map is re-sorted after the build (lane_order rewrites it)
    rq.tc_done = rq.tc_want && n > 0 && !refresh;
    if (rq.tc_done) {
        tb.tc.m = e->m_trav;
        tb.tc.cidx = e->cidx_trav;
        tb.tc.lanes = tb.lanes_remap ? e->lanes_trav : nullptr;
        tb.tc.T = e->T_trav;
        tb.tc.box_header = rq.tc_box;
    }
    // (a build followed by k_trav_inputs forks after that kernel: it reads what the rule writes)
    rq.forked = rq.tc_done && rq.fork_want;
    if (rq.forked) tb.fork_ev = rq.fork_want;
    if (overlap) tb.late_ev = rq.chain_late;
    tb.keys_ready = e->keys_ready && !overlap;
    e->keys_ready = false;
    if (!overlap) e->mir_fresh = false;  // the jitter may move bodies
    HIPCHK(e, tree_build(tb, n, e->geo, s));
    if (e->inject_build >= 0 && e->inject_build-- == 0) {  // bh_debug_inject(2 + k)
        take_u32(tb.scalars + 1, e->scalars + 11, s, 1u);
        HIPCHK(e, hipGetLastError());
    }
    ++e->full_builds;
    e->inv_valid = false;  // the map follows this build's permutation
    if (use_lanes) {
        if (refresh) HIPCHK(e, lane_order(tb, n, e->geo.J, true, e->lanes, s));
        e->lanes_valid = true;
        e->lanes_age = refresh ? 1 : e->lanes_age + 1;
        if (defer && overlap) e->lr_pending = true;
    } else {
        e->lanes_valid = e->lr_pending = e->lr_ready = false;  // this build's permutation was not applied to the map
    }
    e->spl_nb = sort_buckets(n);  // k_prep wrote this build's splitters
    e->st_morton = true;
    if (overlap) return BH_OK;
    if (n > 0) std::swap(e->st, e->alt);
    if (e->solo && n > 0 && !theta2_is_zero(e)) {  // the peers' cell values for later LET builds
        if (!e->solo_table) {
            TRY(dev_alloc(e, e->solo_table, LET_TSTRIDE));
            HIPCHK(e, hipMemsetAsync(e->solo_table, 0, sizeof(LetCell) * LET_TSTRIDE, e->stream));
            TRY(dev_alloc(e, e->solo_all, LET_CELLS));
            TRY(dev_alloc(e, e->solo_cstart, LET_CELLS + 1));
            HIPCHK(e, hipMemsetAsync(e->solo_all, 1, LET_CELLS, e->stream));
        }
        LetBufs Ls{};
        Ls.ecell = e->solo_all;
        Ls.cstart = e->solo_cstart;
        Ls.table = e->solo_table;
        TreeBuffers tm = tree_buffers(e);
        tm.dst = e->st;  // the sorted state
        HIPCHK(e, let_table(n, e->geo, Ls, tm, e->stream));
    }
    e->tree_valid = true;
    return BH_OK;
}

// The velocities left in the previous slot order by a pipelined step (vel_perm) -> st, for any
// reader other than the next step's first kick (materialize_positions calls it: every reader of
// the replica outside the step does that first).
int materialize_velocities(bh_engine *e) {
    if (!e->vel_perm) return BH_OK;
    permute_velocities(e->n, e->vel_perm, e->alt.vx, e->alt.vy, e->st.vx, e->st.vy, e->stream);
    e->vel_perm = nullptr;
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

int build(bh_engine *e) {
    TRY(materialize_velocities(e));
    BuildRequest rq{};  // in place, on the engine's stream, nothing carried or left to others
    return build_into(e, e->stream, rq);
}

// theta = 0 workspace: flags per node slot, selected indices and the leaf list per body.
int ensure_direct(bh_engine *e) {
    if (e->leaf_node_cap == e->node_cap && e->leaf_cap == e->cap) return BH_OK;
    TRY(dev_alloc(e, e->leaf_flags, e->node_cap));
    TRY(dev_alloc(e, e->leaf_sel, (size_t)e->node_cap));
    TRY(dev_alloc(e, e->leaf_count, 1));
    TRY(dev_alloc(e, e->leaf_cover, 2 * ((size_t)e->node_cap + 1)));
    TRY(dev_alloc(e, e->leaves.rec, 4 * (size_t)e->cap));  // (x, y, m, slot) per leaf
    const size_t tb = leaf_select_bytes((int64_t)e->node_cap);
    if (e->leaf_tmp) (void)hipFree(e->leaf_tmp);
    e->leaf_tmp = nullptr;
    HIPCHK(e, hipMalloc(&e->leaf_tmp, tb));
    e->leaf_tmp_bytes = tb;
    e->leaf_node_cap = e->node_cap;
    e->leaf_cap = e->cap;
    return BH_OK;
}

// The previous call's carried tree is used now: its build's error flags become this call's.
int take_carried_flags(bh_engine *e) {
    if (!e->carried_flags) return BH_OK;
    e->carried_flags = false;
    take_u32(e->scalars + 1, e->scalars + 10, e->stream);
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

// ... or it is dropped unused (resetBodies, a root-cell change, a replay).
int drop_carried_flags(bh_engine *e) {
    if (!e->carried_flags) return BH_OK;
    e->carried_flags = false;
    HIPCHK(e, hipMemsetAsync(e->scalars + 10, 0, sizeof(uint32_t), e->stream));
    return BH_OK;
}

// ---- one force evaluation: buildTree() + computeAccelerations() (BHA:359-395) -------------
// theta == 0 (config C5): the criterion never accepts (BHA:226-228), so the force is the
// direct sum over the tree's non-empty leaves in pre-order -- run by the all-pairs kernel
// (direct.hip) on the leaf list instead of the tree walk; bit-identical either way.  The
// visit-counting diagnostic keeps the walk (it counts internal nodes too).
//
// Multi-GPU (e->comm): BH_SHARD_ROUNDS rounds; round k evaluates this rank's piece of the
// Morton order (bh_shard_range) on the compute stream, then the pieces of round k are
// all-gathered in place on the comm stream while round k + 1 is evaluated; the compute
// stream waits for the last gather before the kick.  Pieces of different rounds and ranks
// are disjoint, so the concurrent writes never overlap.
// kick (one GPU, tree walk): the following KDK update is fused into the traversal's epilogue
// and *fused is set; otherwise the caller runs the integration kernel on a2.
#ifndef BH_ROUND_WEIGHTS
#define BH_ROUND_WEIGHTS 1, 1, 1, 1  // relative sizes of a rank's rounds (BH_ROUND_FRACS)
#endif

// ---- multi-rank: the build as a locally essential tree (let.hip) ----------------------
int pinned_reserve(bh_engine *e, size_t bytes);
#ifndef BH_LET_REFRESH
#define BH_LET_REFRESH 32  // LET builds between full builds (the replicated Morton order)
#endif
// s: the stream the set is built on next (the fills of fresh buffers are ordered before it: a
// plain hipMemset is not ordered with the engine's non-blocking streams)
int let_alloc(bh_engine *e, int64_t n_sub, hipStream_t s = nullptr) {
    if (!s) s = e->stream;
    const int J = e->geo.J;
    if (e->let_cap < e->cap || !e->L.ecell) {  // the selection's per-body and per-cell arrays
        const int64_t cap = e->cap;
        LetBufs &L = e->L;
        TRY(dev_alloc(e, L.ecell, LET_CELLS));
        TRY(dev_alloc(e, L.hcell, LET_CELLS));
        TRY(dev_alloc(e, L.flag_all, 1));
        TRY(dev_alloc(e, L.flag8, cap));
        TRY(dev_alloc(e, L.sel, let_sel_blocks(cap) + 2));
        TRY(dev_alloc(e, L.selpos, let_sel_blocks(cap) + 2));
        TRY(dev_alloc(e, e->inv_lanes, cap));
        e->inv_valid = false;
        TRY(dev_alloc(e, L.own, cap));
        TRY(dev_alloc(e, L.own_blk, let_sel_blocks(cap) + 2));
        TRY(dev_alloc(e, L.rowmask, 256 * 8));
        TRY(dev_alloc(e, e->let_box, let_sel_blocks(cap) + 2));
        TRY(dev_alloc(e, e->disp, 2 + (size_t)e->world));
        HIPCHK(e, hipMemsetAsync(e->disp, 0, sizeof(double) * (2 + (size_t)e->world), s));
        L.vmax = reinterpret_cast<unsigned long long *>(e->disp + 1);
        L.nvmax = 1 + e->world;
        e->boxes_valid = false;
        e->let_clean = false;  // (new buffers)
        TRY(alloc_state(e, e->sub_src, cap));
        e->let_cap = cap;
    }
    if (e->set_cap < e->cap || !e->L.cstart) {  // this set's per-cell and per-body arrays
        const int64_t cap = e->cap;
        LetBufs &L = e->L;
        TRY(dev_alloc(e, L.cstart, LET_CELLS + 1));
        TRY(dev_alloc(e, L.table, LET_TSTRIDE));
        TRY(dev_alloc(e, L.tables, (size_t)e->world * LET_TSTRIDE));
        // (solo: the tables of ranks 2 .. world-1 stay zero -- nothing tagged -- for good)
        HIPCHK(e, hipMemsetAsync(L.tables, 0, sizeof(LetCell) * (size_t)e->world * LET_TSTRIDE, s));
        TRY(dev_alloc(e, L.levels, ((size_t)1 << (2 * LET_P + 2)) / 3 + 1));
        TRY(dev_alloc(e, L.w, LET_CELLS + 1));
        TRY(dev_alloc(e, L.posc, LET_CELLS + 1));
        TRY(dev_alloc(e, L.bsz, LET_CELLS + 1));
        TRY(dev_alloc(e, L.csrc, LET_CELLS + 1));
        TRY(dev_alloc(e, L.ccnt, LET_CELLS + 1));
        TRY(dev_alloc(e, L.cpos, LET_CELLS + 1));
        TRY(dev_alloc(e, L.lanes, cap));
        TRY(dev_alloc(e, L.subpos, cap));
        if (!e->table_ev) HIPCHK(e, hipEventCreateWithFlags(&e->table_ev, hipEventDisableTiming));
        e->set_cap = cap;
    }
    e->L.scratch = e->scratch;
    e->L.scratch_bytes = e->scratch_bytes;
    if (n_sub <= e->let_sub_cap && J == e->let_J) return BH_OK;
    // the subset's tree workspace, grown with headroom (the subset drifts between builds)
    const int64_t sc = std::min<int64_t>(e->cap, std::max<int64_t>(n_sub + n_sub / 4, 1024));
    TRY(alloc_state(e, e->sub_dst, sc));
    TRY(dev_alloc(e, e->s_keys, sc));
    TRY(dev_alloc(e, e->s_keys_s, sc));
    TRY(dev_alloc(e, e->s_keys32, sc));
    TRY(dev_alloc(e, e->s_keys32_s, sc));
    TRY(dev_alloc(e, e->s_idx, sc));
    TRY(dev_alloc(e, e->s_perm, sc));
    TRY(dev_alloc(e, e->s_cpl, sc + 32));
    TRY(dev_alloc(e, e->s_cnt, sc + 1));
    TRY(dev_alloc(e, e->s_base, sc + 1));
    TRY(dev_alloc(e, e->s_cell_start, ((size_t)1 << (2 * std::min(J, CELL_TABLE_MAX_DEPTH))) + 2));
    const size_t ncap = node_capacity(sc, J);
    TRY(dev_alloc(e, e->s_nodes, ncap));
    e->let_node_cap = ncap + 2 * (size_t)LET_CELLS + 64;
    TRY(dev_alloc(e, e->L.nodes, e->let_node_cap));
    e->L.node_cap = (uint32_t)std::min<size_t>(e->let_node_cap, 0xFFFFFFF0u);
    TRY(dev_alloc(e, e->s_span_list, (size_t)(J + 2) * span_stride_for(sc)));
    TRY(dev_alloc(e, e->s_span_children, (size_t)(J + 2) * span_stride_for(sc)));
    TRY(dev_alloc(e, e->s_super_list, (size_t)(J + 2) * span_groups(span_stride_for(sc))));
    TRY(dev_alloc(e, e->s_spl, (size_t)sort_buckets(sc) + 2));
    TRY(dev_alloc(e, e->s_bcount, (size_t)sort_buckets(sc) + 2));
    TRY(dev_alloc(e, e->s_bstart, (size_t)sort_buckets(sc) + 2));
    HIPCHK(e, hipMemsetAsync(e->s_bcount, 0, sizeof(uint32_t) * ((size_t)sort_buckets(sc) + 2), s));
    e->s_spl_nb = 0;
    e->let_sub_cap = sc;
    e->let_J = J;
    return BH_OK;
}

TreeBuffers let_tree_buffers(bh_engine *e) {
    TreeBuffers b;
    b.src = e->sub_src;
    b.src.vy = nullptr;  // (a subset's vx carries the replicated slot; its vy is never read)
    b.dst = e->sub_dst;
    b.keys = e->s_keys;
    b.keys_s = e->s_keys_s;
    b.keys32 = e->s_keys32;
    b.keys32_s = e->s_keys32_s;
    b.idx = e->s_idx;
    b.perm = e->s_perm;
    b.cpl = e->s_cpl;
    b.cnt = e->s_cnt;
    b.base = e->s_base;
    b.cell_start = e->s_cell_start;
    b.nodes = e->s_nodes;
    b.scalars = e->scalars;
    b.span_list = e->s_span_list;
    b.span_stride = span_stride_for(e->let_sub_cap);
    b.span_children = e->s_span_children;
    b.super_list = e->s_super_list;
    b.scratch = e->scratch;
    b.scratch_bytes = e->scratch_bytes;
    b.spl = e->s_spl;
    // the subset is compacted from the Morton-ordered state, nearly sorted: the adaptive bucket
    // sort with the previous LET build's splitters (any splitters partition correctly)
    b.spl_nb = e->s_spl_nb;
    b.bcount = e->s_bcount;
    b.bstart = e->s_bstart;
    return b;
}

// LET subset capacity: the largest subset seen + headroom (a subset beyond it replays the call)
#ifndef BH_LET_HEADROOM_SHIFT
#define BH_LET_HEADROOM_SHIFT 3
#endif
inline int64_t let_capacity(int64_t known) {
    return known + (known >> BH_LET_HEADROOM_SHIFT) + 4096;
}
#ifndef BH_LET_MIN_WORLD
#define BH_LET_MIN_WORLD 2
#endif
bool let_active(const bh_engine *e) {
    return e->let_on && (e->let_forced || e->world >= BH_LET_MIN_WORLD);
}

// Stream of round k (even: the engine's stream; odd: stream2, started after the build).
int round_streams(bh_engine *e) {
    if (!e->stream2) {
        HIPCHK(e, hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
        HIPCHK(e, hipEventCreateWithFlags(&e->built_ev, hipEventDisableTiming));
    }
    HIPCHK(e, hipEventRecord(e->built_ev, e->stream));
    HIPCHK(e, hipStreamWaitEvent(e->stream2, e->built_ev, 0));
    return BH_OK;
}

// Round k's in-place all-gather of W doubles per lane on the comm stream (RCCL), or the peers'
// pieces copied in (in-process group: the caller has passed a barrier after every member
// recorded round_ev[ev_round]; ev_round < 0: the peers' events were waited for already).
bool solo_xchg_on() {
    static const bool on = [] {
        const char *v = std::getenv("BH_SOLO_XCHG");
        return v && std::strcmp(v, "0") != 0;
    }();
    return on;
}

int gather_round(bh_engine *e, const GatherLayout &gl, int k, int W, int ev_round, int site) {
    const int64_t size = gl.off[k + 1] - gl.off[k];
    double *piece = e->a2 + W * (int64_t)e->world * gl.off[k];  // round k, rank 0
    if (size <= 0) return BH_OK;
    TRY(coll_log(e, site, (int64_t)sizeof(double) * W * size * e->world, CS_COMM));
    if (e->comm) {
        NCCLCHK(e, ncclAllGather(piece + W * e->rank * size, piece, (size_t)(W * size),
                                 ncclDouble, e->comm, e->comm_stream));
    } else if (e->solo && e->world > 1 && solo_xchg_on()) {
        // measurement only (tools/solo_rank.py): the bytes a rank receives per round, as one
        // device copy of the own piece on the comm stream -- the copy kernel competes for wave
        // slots with the traversal rounds the way the all-gather's kernel would; peers' positions
        // stay where they are (the copy goes to a scratch buffer)
        const int64_t need = (int64_t)W * size * (e->world - 1);
        if (e->solo_xchg_cap < need) {
            TRY(dev_alloc(e, e->solo_xchg, (size_t)need));
            e->solo_xchg_cap = need;
        }
        for (int q = 1; q < e->world; ++q)
            HIPCHK(e, hipMemcpyAsync(e->solo_xchg + (int64_t)W * size * (q - 1),
                                     piece + W * e->rank * size, sizeof(double) * W * size,
                                     hipMemcpyDeviceToDevice, e->comm_stream));
    } else if (e->group) {
        for (int q = 0; q < e->world; ++q) {
            if (q == e->rank) continue;
            bh_engine *peer = e->group->members[q];
            if (ev_round >= 0)
                HIPCHK(e, hipStreamWaitEvent(e->comm_stream, peer->round_ev[ev_round], 0));
            const int64_t off = W * ((int64_t)e->world * gl.off[k] + q * size);
            HIPCHK(e, hipMemcpyAsync(e->a2 + off, peer->a2 + off, sizeof(double) * W * size,
                                     hipMemcpyDeviceToDevice, e->comm_stream));
        }
    }
    return BH_OK;
}

// The positions a sequence of LET evaluations left in the exchange buffer -> the replica (every
// body's slot), before anything but the next selection reads x, y (a full build, the merge rule,
// the copy-out) or reuses a2 (accelerations, the velocity exchange).  A subset overflow (scalars[4],
// the call is replayed) leaves the replica as it was.
int materialize_positions(bh_engine *e) {
    TRY(materialize_velocities(e));
    if (!e->pos_pending) return BH_OK;
    e->pos_pending = false;
    if (e->n <= 0) return BH_OK;
    let_set_pos(e->n, e->pos_lanes, e->a2, e->pos_layout, e->st.x, e->st.y, e->scalars + 4,
                e->stream);
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

// Velocities after owner-integrated LET evaluations: every rank holds current velocities of its
// own bodies only; before a full build (which permutes and re-assigns the bodies) the owners'
// (vx, vy) are all-gathered once, in the same rounds and slots as the forces.
int sync_velocities(bh_engine *e) {
    if (!e->vel_stale) return BH_OK;
    e->vel_stale = false;
    const int64_t n = e->n;
    if (n <= 0 || e->solo) return BH_OK;  // solo: no peers (their bodies keep their velocities)
    const int R = BH_SHARD_ROUNDS;
    const int64_t sub = shard_sub(n, e->world, R);
    const uint32_t *lanes = e->lanes_valid ? e->lanes : nullptr;
    const LetPieces pc{n, sub, e->world, e->rank, R, lanes};
    const GatherLayout gl = shard_layout(n, e->world);
    if (e->group) {  // peers are done reading our previous pieces
        TRY(group_barrier(e));
        for (bh_engine *peer : e->group->members)
            if (peer != e) HIPCHK(e, hipStreamWaitEvent(e->stream, peer->gathered_ev, 0));
    }
    let_pack_vel(pc, e->st.vx, e->st.vy, e->a2, gl, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->round_ev[0], e->stream));
    HIPCHK(e, hipStreamWaitEvent(e->comm_stream, e->round_ev[0], 0));
    if (e->group) TRY(group_barrier(e));
    for (int k = 0; k < R; ++k) TRY(gather_round(e, gl, k, 2, k == 0 ? 0 : -1, COLL_VEL));
    HIPCHK(e, hipEventRecord(e->gathered_ev, e->comm_stream));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->gathered_ev, 0));
    let_unpack_vel(n, lanes, e->a2, gl, e->st.vx, e->st.vy, e->stream);
    HIPCHK(e, hipGetLastError());
    return BH_OK;
}

// One LET evaluation with its integration (kick: KICK_DRIFT after a(t), KICK_ONLY after
// a(t+dt)); *done = false when it does not apply (the caller builds the full tree).  Each lane
// kicks its own body (velocity in the replicated state, owner only) and sends the body's new
// position -- drifted, or as the build left it (jitter, BHA:146-151) -- so every replica takes
// all positions from the exchange.
int wave_order_for(bh_engine *e, int slot, int64_t lanes, hipStream_t s, WaveOrder &wo);
int wave_order_next(bh_engine *e, int slot, int64_t lanes, hipStream_t s);

// Every rank's LET cell table into L.tables, on stream s.  RCCL: one all-gather on the engine's
// stream.  In-process group: each member publishes its table and event, then copies every
// member's.
int exchange_tables(bh_engine *e, hipStream_t s) {
    const size_t tbytes = sizeof(LetCell) * (size_t)LET_TSTRIDE;
    TRY(coll_log(e, COLL_TABLE, (int64_t)(tbytes * (size_t)e->world), CS_MAIN));
    if (e->comm) {
        NCCLCHK(e, ncclAllGather(e->L.table, e->L.tables, tbytes, ncclUint8, e->comm, s));
    } else if (e->solo) {  // own values first, the rest from the last full build
        HIPCHK(e, hipMemcpyAsync(e->L.tables, e->L.table, tbytes, hipMemcpyDeviceToDevice, s));
        if (e->world > 1 && e->solo_table)
            HIPCHK(e, hipMemcpyAsync(e->L.tables + LET_TSTRIDE, e->solo_table, tbytes,
                                     hipMemcpyDeviceToDevice, s));
    } else {
        // (a member reads the published pointers after the barrier; it publishes again only
        // after the round barriers that follow, which every member passes first)
        e->pub_table = e->L.table;
        e->pub_table_ev = e->table_ev;
        HIPCHK(e, hipEventRecord(e->table_ev, s));
        TRY(group_barrier(e));
        for (int q = 0; q < e->world; ++q) {
            bh_engine *peer = e->group->members[q];
            if (peer != e) HIPCHK(e, hipStreamWaitEvent(s, peer->pub_table_ev, 0));
            HIPCHK(e, hipMemcpyAsync(e->L.tables + (size_t)q * LET_TSTRIDE, peer->pub_table, tbytes,
                                     hipMemcpyDeviceToDevice, s));
        }
    }
    return BH_OK;
}

// Every rank's drift speed bound (its own bodies' max |v| after the kick, L.vmax[0]) into
// L.vmax[1 + rank], on the exchange stream behind the rounds (which it waited for): RCCL, or the
// peers' words copied (in-process group).  A solo rank has no peers: its own word is the bound.
int gather_vmax(bh_engine *e) {
    TRY(coll_log(e, COLL_VMAX, (int64_t)sizeof(unsigned long long) * e->world, CS_COMM));
    if (e->comm) {
        NCCLCHK(e, ncclAllGather(e->L.vmax, e->L.vmax + 1, 1, ncclUint64, e->comm,
                                 e->comm_stream));
    } else if (e->group) {
        for (bh_engine *peer : e->group->members)
            if (peer != e)
                HIPCHK(e, hipMemcpyAsync(e->L.vmax + 1 + peer->rank, peer->L.vmax,
                                         sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                                         e->comm_stream));
    }
    return BH_OK;
}

int evaluate_let(bh_engine *e, KickMode kick, bool *done) {
    *done = false;
    if (kick != KICK_DRIFT && kick != KICK_ONLY) return BH_OK;
    const int64_t n = e->n;
    const double gap2 = let_include_gap2(e->geo, e->p.theta * e->p.theta, e->p.soft2);
    if (gap2 < 0.0 || n <= 0) return BH_OK;
    const int R = BH_SHARD_ROUNDS;
    const int64_t sub = shard_sub(n, e->world, R);
    // the pieces are lane ranges of the Hilbert wave map when it is current (as in the full
    // path), else slot ranges; a2 is written by lane either way
    const uint32_t *lanes = e->lanes_valid ? e->lanes : nullptr;
    const LetPieces pc{n, sub, e->world, e->rank, R, lanes};
    TRY(mark(e, -1));
    if (e->group) {  // peers are done reading our previous table and pieces
        TRY(group_barrier(e));
        for (bh_engine *peer : e->group->members)
            if (peer != e) HIPCHK(e, hipStreamWaitEvent(e->stream, peer->gathered_ev, 0));
    }
    int64_t n_sub = 0;
    {
        TRY(let_alloc(e, 0));
        // subset capacity: the largest subset of the previous call + headroom, no host round trip;
        // a subset beyond it is an overflow every rank sees after the exchange, and bh_step replays
        // the call with the observed size (the first LET build of an engine reads its size once)
        // (the selection writes sub_src, sized for the whole state; padding up to S = n is harmless).
        // Within a call the size follows the previous selection's when its read-back has landed
        // (a contracting cloud's subsets grow by more than the headroom over a 100-step call:
        // round 4 saw one replay of the C4 / 8 call).  Never waited for: a blocking wait here cost
        // 0.2 ms per solo C4 / 8 step (3.67 against 3.43-3.53 ms).
        if (e->let_known > 0 && e->sub_cnt_pending && hipEventQuery(e->sub_cnt_ev) == hipSuccess) {
            e->sub_cnt_pending = false;
            e->let_known = std::max<int64_t>(e->let_known, *e->sub_cnt_h);
        }
        int64_t S = e->let_known > 0 ? std::min<int64_t>(n, let_capacity(e->let_known)) : n;
        PosSrc ps{nullptr, GatherLayout{}, nullptr};
        if (e->pos_pending && lanes != e->pos_lanes) TRY(materialize_positions(e));  // map changed
        if (e->pos_pending) {  // the previous LET evaluation's positions, straight from a2
            if (!e->inv_valid) {  // per lane map: each slot's position in the exchange buffer
                let_gather_slots(n, lanes, e->pos_layout, e->inv_lanes, e->stream);
                HIPCHK(e, hipGetLastError());
                e->inv_valid = true;
            }
            ps = PosSrc{e->a2, e->pos_layout, e->inv_lanes};
        }
        // the subset build's keys and buckets from the gather when its buffers and splitters are
        // those of the previous LET build (same S capacity and J; not the first build, which sorts
        // with rocprim and sizes the subset afterwards)
        // a grown capacity S: splitters for its new padding tail (else one bucket takes it all
        // and sorts it alone: up to 1 ms per build while the call's largest subset still grows)
        if (e->s_spl_nb > 0 && S <= e->let_sub_cap && e->geo.J == e->let_J &&
            sort_buckets(S) > e->s_spl_nb) {
            extend_splitters(e->s_spl, e->s_spl_nb, sort_buckets(S), e->geo.J, e->stream);
            HIPCHK(e, hipGetLastError());
            e->s_spl_nb = sort_buckets(S);
        }
        MortonFuse mf{};
        const bool fuse = e->let_known > 0 && e->s_spl_nb > 0 &&
                          S <= e->let_sub_cap && e->geo.J == e->let_J && e->s_keys;
        if (fuse)
            mf = MortonFuse{e->s_keys, e->s_keys32, e->s_spl, e->s_spl_nb, e->s_cnt, e->s_base,
                            e->s_bcount};
        // only the slot blocks that may hold a body of a built cell (LetSweep): the jitter of
        // every build since the boxes moved a body by at most 2 x 2e-3 per axis (BHA:146-151)
        const LetSweep sw{e->let_box, e->disp, 4.0e-3 * (double)(e->builds_since_box + 1),
                          e->boxes_valid};
        HIPCHK(e, let_select(e->st, ps, e->geo, pc, gap2, e->L, e->sub_src, S, e->scalars,
                             e->stream, mf, sw, e->let_clean && e->let_clean_n == n));
        e->let_clean = false;
        ++e->builds_since_box;
        if (e->let_known > 0) {
            if (!e->sub_cnt_h) {
                HIPCHK(e, hipHostMalloc((void **)&e->sub_cnt_h, 64, hipHostMallocDefault));
                HIPCHK(e, hipEventCreateWithFlags(&e->sub_cnt_ev, hipEventDisableTiming));
            }
            HIPCHK(e, hipMemcpyAsync(e->sub_cnt_h, e->L.selpos + let_sel_blocks(n),
                                     sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(e, hipEventRecord(e->sub_cnt_ev, e->stream));
            e->sub_cnt_pending = true;
        }
        if (e->let_known <= 0) {
            TRY(pinned_reserve(e, 64));
            uint32_t *h = static_cast<uint32_t *>(e->pin);
            HIPCHK(e, hipMemcpyAsync(h, e->L.selpos + let_sel_blocks(n), sizeof(uint32_t), hipMemcpyDeviceToHost,
                                     e->stream));
            SYNC(e, e->stream);
            e->let_known = std::max<int64_t>(h[0], 1);
            S = std::min<int64_t>(n, let_capacity(e->let_known));  // padded above
        }
        TRY(let_alloc(e, S));
        n_sub = S;  // padded: bodies past the real subset are dead
        ++e->let_builds;
        TreeBuffers sb = let_tree_buffers(e);
        sb.keys_ready = fuse && e->s_spl_nb > 0;  // (let_alloc above kept the buffers: S fitted)
        HIPCHK(e, tree_build(sb, n_sub, e->geo, e->stream));
        e->s_spl_nb = sort_buckets(n_sub);  // k_prep wrote this build's splitters
        HIPCHK(e, let_table(n_sub, e->geo, e->L, sb, e->stream));
        TRY(exchange_tables(e, e->stream));
        {
            // bh_debug_inject: a node array of one record makes k_let_guard fire on this rank only,
            // exactly as a broken invariant would (empty tree, idle lanes, replay flag set)
            const uint32_t node_cap = e->L.node_cap;
            if (e->inject_guard) e->L.node_cap = 1u;
            e->inject_guard = false;
            const hipError_t rc = let_assemble(n_sub, e->geo, pc, e->L, sb, e->scalars, e->stream,
                                               &e->let_clean);
            e->let_clean_n = n;
            e->L.node_cap = node_cap;
            HIPCHK(e, rc);
        }
    }
    TRY(mark(e, 0));
    const ForceParams fp = force_params(e);
    const int W = 2;  // (x, y) per lane
    KickArgs ka{kick == KICK_DRIFT ? KICK_OWN_DRIFT : KICK_OWN_ONLY, e->st.vx, e->st.vy,
                e->p.dt * 0.5, e->p.dt, lanes};  // BHA:412
    const bool bound = kick == KICK_DRIFT && e->boxes_valid;  // the drift's speed bound
    if (bound) ka.vmax = e->L.vmax;
    const GatherLayout gl = shard_layout(n, e->world);
    // measurement: the peers' bodies keep their positions (already in a2 after a LET evaluation)
    if (e->solo && !e->pos_pending) let_fill_pos(n, lanes, e->st.x, e->st.y, e->a2, gl, e->stream);
    TRY(round_streams(e));
    for (int k = 0; k < R; ++k) {
        int64_t lo = 0, hi = 0;
        bh_shard_range(n, e->rank, e->world, k, &lo, &hi);
        hipStream_t rs = (k & 1) ? e->stream2 : e->stream;
        // lane q of the piece writes slot gather_slot(q) = q - lo + gather_slot(lo)
        double *a2r = e->a2 + W * (gather_slot(gl, lo) - lo);
        WaveOrder wo;
        TRY(wave_order_for(e, 1 + k, hi - lo, rs, wo));
        traverse(e->L.nodes, e->let_node_cap, e->L.posc + LET_CELLS, e->sub_dst.x, e->sub_dst.y,
                 e->sub_dst.m, e->sub_dst.cidx, lo, hi, e->geo, fp, a2r, nullptr, rs,
                 &ka, e->L.lanes, &wo);
        HIPCHK(e, hipGetLastError());
        TRY(wave_order_next(e, 1 + k, hi - lo, rs));
        HIPCHK(e, hipEventRecord(e->round_ev[k], rs));
        HIPCHK(e, hipStreamWaitEvent(e->comm_stream, e->round_ev[k], 0));
        if (e->group) TRY(group_barrier(e));
        TRY(gather_round(e, gl, k, W, k, COLL_POS));
    }
    if (bound) TRY(gather_vmax(e));  // behind the last round, on the exchange stream
    TRY(mark(e, 1));
    HIPCHK(e, hipEventRecord(e->gathered_ev, e->comm_stream));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->gathered_ev, 0));
    if (bound) {  // the bound now covers every rank's drift
        let_disp_add(e->disp, e->L.vmax, e->L.nvmax, e->p.dt, e->stream);
        HIPCHK(e, hipGetLastError());
    }
    TRY(mark(e, 4));
    e->pos_pending = true;  // every body's new position is in a2 (by lane, gather slots)
    e->pos_lanes = lanes;
    e->pos_layout = gl;
    e->vel_stale = true;
    e->a2_lanes = lanes;
    e->a2_layout = gl;
    e->tree_valid = false;  // the full tree was not built
    *done = true;
    return BH_OK;
}

// Longest-first wave dispatch for a one-GPU traversal over all n lanes (traverse.hip).
#ifndef BH_TRAV_LPT
#define BH_TRAV_LPT 0  // measured without gain; the wave durations stay recordable
#endif
// The order for the next launch is made right after each launch (wave_order_next), off the
// traversal's timed interval; a launch over another lane count first makes its own.
// slot: 0 for the one-GPU launch, 1 + k for LET round k; lanes: the launch's lane count.
// Below BH_LPT_MIN_LANES every wave starts at once anyway (8192 wave slots per GPU).
#ifndef BH_LPT_MIN_LANES
#define BH_LPT_MIN_LANES 131072
#endif
bool wave_order_used(int64_t lanes) {
    return BH_TRAV_LPT && lanes >= BH_LPT_MIN_LANES && wave_order_runs(lanes) != 0;
}

int wave_order_for(bh_engine *e, int slot, int64_t lanes, hipStream_t s, WaveOrder &wo) {
    wo = WaveOrder{};
    if (!wave_order_used(lanes)) return BH_OK;
    uint32_t *cost = e->wave_cost + slot * e->cost_stride;
    uint32_t *order = e->run_order + slot * e->order_stride;
    if (e->order_n[slot] != lanes) {  // the order must be a permutation of this launch's runs
        HIPCHK(e, wave_order(cost, lanes, order, s));
        e->order_n[slot] = lanes;
    }
    wo.order = order;
    wo.cost = cost;
    return BH_OK;
}

int wave_order_next(bh_engine *e, int slot, int64_t lanes, hipStream_t s) {
    if (!BH_TRAV_LPT || lanes <= 0 || e->order_n[slot] != lanes) return BH_OK;
    HIPCHK(e, wave_order(e->wave_cost + slot * e->cost_stride, lanes,
                         e->run_order + slot * e->order_stride, s));
    return BH_OK;
}

// The full tree of the current state, for a force evaluation or a query: the one the pipelined
// step carried into this call (with its build's flags; its jitter becomes part of the state), or a
// build now -- never a LET, not sharded.  Afterwards e->nodes, e->base[n] (the node count) and
// e->st in the build's slot order are current on e->stream.
int ensure_tree(bh_engine *e) {
    e->let_age = 0;
    const int64_t n = e->n;
    if (e->prebuilt) {  // the pipelined step built this tree (single GPU: nothing deferred)
        e->prebuilt = false;
        TRY(take_carried_flags(e));
        e->view_pending = false;  // its jitter is now part of the state (BHA:146-151)
        e->mir_fresh = false;
    } else {
        TRY(materialize_positions(e));  // the replica's x, y; a2 is free again
        TRY(sync_velocities(e));        // before the full build permutes the state
        TRY(mark(e, -1));
        TRY(build(e));
        if ((e->comm || e->group || e->solo) && let_active(e) && !theta2_is_zero(e) && n > 0) {
            // the LET selections until the next full build scan only the slot blocks whose box
            // (the cells of their bodies now, in this build's slot order) may reach a built cell
            TRY(let_alloc(e, 0));
            let_boxes(n, e->st, e->geo, e->let_box, e->stream);
            HIPCHK(e, hipGetLastError());
            HIPCHK(e, hipMemsetAsync(e->disp, 0, sizeof(double), e->stream));
            e->boxes_valid = true;
            e->builds_since_box = 0;
        }
        TRY(mark(e, 0));
    }
    return BH_OK;
}

// The tree's non-empty leaves in pre-order into e->leaves (the all-pairs kernels' input).
int build_leaf_list(bh_engine *e) {
    TRY(ensure_direct(e));
    HIPCHK(e, leaf_list_build(e->nodes, e->base + e->n, (int64_t)e->node_cap, e->leaf_flags,
                              e->leaf_sel, e->leaf_count, e->leaves, e->n, e->leaf_cover,
                              e->leaf_tmp, e->leaf_tmp_bytes, e->stream));
    return BH_OK;
}

// ---- the queries' launches --------------------------------------------------------------
// Each runs on the tree ensure_tree() left (tree = false: no bodies, no tree -- every sum stays
// +0.0), by this engine alone, into buffers of its own that are made on first use and grown when
// needed, with its kernel between the two events of its stopwatch.  None touches a2, the state
// or what the pipelined step carries into the next call.
int potential_bufs(bh_engine *e) {
    if (outgrown(e->phi_cap, e->phi, e->cap)) {
        TRY(dev_alloc(e, e->phi, (size_t)e->cap));
        e->phi_cap = e->cap;
    }
    if (!e->diag_part) TRY(dev_alloc(e, e->diag_part, diag_partial_doubles()));
    return BH_OK;
}

// bh_compute_potential: the potential of every body into e->phi, by slot.
int potential_launch(bh_engine *e) {
    const int64_t n = e->n;
    const ForceParams fp = force_params(e);
    TRY(potential_bufs(e));
    if (fp.theta2 == 0.0) {  // all pairs over the leaf sequence (direct.hip)
        TRY(build_leaf_list(e));
        TRY(e->pot_sw.start(e, e->stream));
        direct_potential(e->leaves, e->leaf_count, e->st.x, e->st.y, e->st.cidx, n, fp.G, fp.soft2,
                         e->phi, e->stream);
    } else {
        TRY(e->pot_sw.start(e, e->stream));
        potential_walk(e->nodes, e->node_cap, e->base + n, e->st.x, e->st.y, e->st.cidx, n, e->geo,
                       fp, e->phi, e->lanes_valid ? e->lanes : nullptr, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    return e->pot_sw.stop(e, e->stream);
}

// The caller's probes of bh_compute_field / bh_compute_field_direct (host arrays; pm nullable).
struct Probes {
    int64_t n;
    const double *px, *py, *pm;
};

int upload_probes(bh_engine *e, const Probes &p, double *px, double *py, double *pm) {
    const size_t bytes = sizeof(double) * (size_t)p.n;
    HIPCHK(e, hipMemcpyAsync(px, p.px, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(py, p.py, bytes, hipMemcpyHostToDevice, e->stream));
    if (pm) HIPCHK(e, hipMemcpyAsync(pm, p.pm, bytes, hipMemcpyHostToDevice, e->stream));
    return BH_OK;
}

// bh_compute_field: upload, key and sort the probes, then the field walk (theta = 0: the same
// walk, which then opens every internal node) into e->fld_out by probe index.
int field_launch(bh_engine *e, const Probes &p, bool tree) {
    const int64_t P = p.n;
    if (outgrown(e->fld_cap, e->fld_in, P)) {
        const size_t cap = (size_t)P;
        TRY(dev_alloc(e, e->fld_in, 3 * cap));   // px, py, pm
        TRY(dev_alloc(e, e->fld_out, 3 * cap));  // ax, ay, phi
        TRY(dev_alloc(e, e->fld_u32, 4 * cap));  // key, sorted key, index, order
        if (e->fld_scratch) (void)hipFree(e->fld_scratch);
        e->fld_scratch = nullptr;
        e->fld_scratch_bytes = field_sort_bytes(P);
        HIPCHK(e, hipMalloc(&e->fld_scratch, e->fld_scratch_bytes ? e->fld_scratch_bytes : 1));
        e->fld_cap = P;
    }
    const size_t cap = (size_t)e->fld_cap;
    double *px = e->fld_in, *py = px + cap, *pm = p.pm ? py + cap : nullptr;
    TRY(upload_probes(e, p, px, py, pm));
    uint32_t *key = e->fld_u32, *key_s = key + cap, *idx = key_s + cap, *order = idx + cap;
    HIPCHK(e, field_order(P, px, py, e->geo, key, key_s, idx, order, e->fld_scratch,
                          e->fld_scratch_bytes, e->stream));
    TRY(e->fld_sw.start(e, e->stream));
    field_walk(tree ? e->nodes : nullptr, tree ? e->node_cap : 0, tree ? e->base + e->n : nullptr,
               px, py, pm, order, P, e->geo, force_params(e), e->fld_out, e->fld_out + cap,
               e->fld_out + 2 * cap, e->stream);
    HIPCHK(e, hipGetLastError());
    return e->fld_sw.stop(e, e->stream);
}

// The targets' planes of k_direct_targets: tx, ty, tm; ax, ay, phi, ax_tree, ay_tree; the
// samples' caller indices and their slots.
int direct_field_bufs(bh_engine *e, int64_t n_target) {
    if (outgrown(e->dfl_cap, e->dfl_in, n_target)) {
        const size_t cap = (size_t)n_target;
        TRY(dev_alloc(e, e->dfl_in, 3 * cap));
        TRY(dev_alloc(e, e->dfl_out, 5 * cap));
        TRY(dev_alloc(e, e->dfl_u32, 2 * cap));
        e->dfl_cap = n_target;
    }
    return BH_OK;
}

// bh_compute_field_direct: every leaf of the tree's leaf sequence summed by the tiled kernel
// (direct_field.hip) into e->dfl_out by probe index, whatever theta is -- no cell is accepted.
int direct_field_launch(bh_engine *e, const Probes &p, bool tree) {
    const int64_t P = p.n;
    const ForceParams fp = force_params(e);
    if (tree) TRY(build_leaf_list(e));
    TRY(direct_field_bufs(e, P));
    const size_t cap = (size_t)e->dfl_cap;
    double *px = e->dfl_in, *py = px + cap, *pm = p.pm ? py + cap : nullptr;
    TRY(upload_probes(e, p, px, py, pm));
    TRY(e->dfl_sw.start(e, e->stream));
    direct_targets(tree ? e->leaves : LeafList{nullptr}, tree ? e->leaf_count : nullptr, px, py, pm,
                   nullptr, P, fp.G, fp.soft2, e->dfl_out, e->dfl_out + cap, e->dfl_out + 2 * cap,
                   e->stream);
    HIPCHK(e, hipGetLastError());
    return e->dfl_sw.stop(e, e->stream);
}

// bh_compute_field_grid: the probes are the grid's points, formed by k_field_grid itself, into
// the planes of e->fgr_out that `planes` names (bit k: ax, ay, phi; all three with stats), then
// -- with stats -- their summary into e->fgr_stats.  There is nothing to upload.
int field_grid_launch(bh_engine *e, const bh_field_grid &g, unsigned planes, bool stats,
                      bool tree) {
    const int64_t points = (int64_t)g.nx * g.ny;
    if (outgrown(e->fgr_cap, e->fgr_out, points)) {
        TRY(dev_alloc(e, e->fgr_out, 3 * (size_t)points));
        e->fgr_cap = points;
    }
    if (!e->fgr_stats) TRY(dev_alloc(e, e->fgr_stats, field_grid_stat_partials()));
    const size_t cap = (size_t)e->fgr_cap;
    double *out[3];
    for (int k = 0; k < 3; ++k)
        out[k] = (stats || (planes >> k & 1u)) ? e->fgr_out + k * cap : nullptr;
    TRY(e->fgr_sw.start(e, e->stream));
    field_grid_walk(tree ? e->nodes : nullptr, tree ? e->node_cap : 0,
                    tree ? e->base + e->n : nullptr, g, e->geo, force_params(e), out[0], out[1],
                    out[2], e->stream);
    HIPCHK(e, hipGetLastError());
    TRY(e->fgr_sw.stop(e, e->stream));
    if (stats) {
        field_grid_stats(points, out[0], out[1], out[2], e->fgr_stats,
                         e->fgr_stats + field_grid_stat_partials() - 1, e->stream);
        HIPCHK(e, hipGetLastError());
    }
    return BH_OK;
}

// The caller's arguments of bh_find_neighbors (host arrays; pr nullable), what it asked for, and
// what the launch found out.
struct NeighborQuery {
    int64_t n;
    const double *px, *py, *pr;
    double r;
    bool counting;  // counts (and with them offsets and the total) are wanted
    bool nearest;   // nearest / d2_nearest are wanted
    bool lists;     // offsets and indices are wanted, `cap` entries of room
    int64_t cap;
    int64_t total = 0;    // neighbours in all (counting)
    bool filled = false;  // the lists were written: total <= cap
};

// The planes of e->nbr_i64: count and offsets of nbr_cap + 1 entries each, then nearest.
struct NeighborPlanes {
    int64_t *count, *offsets, *nearest;
};
NeighborPlanes neighbor_planes(const bh_engine *e) {
    const size_t cap1 = (size_t)e->nbr_cap + 1;
    return NeighborPlanes{e->nbr_i64, e->nbr_i64 + cap1, e->nbr_i64 + 2 * cap1};
}

// bh_find_neighbors: upload, key and sort the probes as bh_compute_field does, then the radius
// walk for counts and nearest, the scan of the counts and -- if lists are asked for and fit -- the
// second walk and the segmented sort, all into the engine's own planes.  The stopwatch runs from
// the first walk to the last kernel; with lists it spans the read-back of the total in between.
int neighbors_launch(bh_engine *e, NeighborQuery &q, bool tree) {
    const int64_t P = q.n;
    if (outgrown(e->nbr_cap, e->nbr_in, P)) {
        const size_t cap = (size_t)P;
        TRY(dev_alloc(e, e->nbr_in, 3 * cap));       // px, py, pr
        TRY(dev_alloc(e, e->nbr_u32, 4 * cap));      // key, sorted key, index, order
        TRY(dev_alloc(e, e->nbr_i64, 3 * cap + 2));  // count, offsets, nearest
        TRY(dev_alloc(e, e->nbr_d2, cap));
        if (e->nbr_scratch) (void)hipFree(e->nbr_scratch);
        e->nbr_scratch = nullptr;
        e->nbr_scratch_bytes = std::max(field_sort_bytes(P), neighbors_scan_bytes(P));
        HIPCHK(e, hipMalloc(&e->nbr_scratch, e->nbr_scratch_bytes ? e->nbr_scratch_bytes : 1));
        e->nbr_cap = P;
    }
    const size_t cap = (size_t)e->nbr_cap;
    double *px = e->nbr_in, *py = px + cap, *pr = q.pr ? py + cap : nullptr;
    TRY(upload_probes(e, Probes{P, q.px, q.py, q.pr}, px, py, pr));
    uint32_t *key = e->nbr_u32, *key_s = key + cap, *idx = key_s + cap, *order = idx + cap;
    HIPCHK(e, field_order(P, px, py, e->geo, key, key_s, idx, order, e->nbr_scratch,
                          e->nbr_scratch_bytes, e->stream));
    const NeighborPlanes pl = neighbor_planes(e);
    const Node *nodes = tree ? e->nodes : nullptr;
    const size_t node_cap = tree ? e->node_cap : 0;
    const uint32_t *d_T = tree ? e->base + e->n : nullptr;
    const uint32_t *cidx = tree ? e->st.cidx : nullptr;
    const NeighborReach rc = neighbor_reach_terms(e->geo);
    if (q.counting) HIPCHK(e, hipMemsetAsync(pl.count + P, 0, sizeof(int64_t), e->stream));
    TRY(e->nbr_sw.start(e, e->stream));
    neighbors_count(nodes, node_cap, d_T, cidx, px, py, pr, q.r, order, P, rc,
                    q.counting ? pl.count : nullptr, q.nearest ? pl.nearest : nullptr, e->nbr_d2,
                    e->stream);
    HIPCHK(e, hipGetLastError());
    if (q.counting) {
        HIPCHK(e, neighbors_offsets(P, pl.count, pl.offsets, e->nbr_scratch, e->nbr_scratch_bytes,
                                    e->stream));
        HIPCHK(e, hipMemcpyAsync(&q.total, pl.offsets + P, sizeof(int64_t), hipMemcpyDeviceToHost,
                                 e->stream));
        SYNC(e, e->stream);
    }
    if (q.lists && q.total <= q.cap && q.total > 0) {
        if (q.total > (int64_t)INT32_MAX) {
            e->err = "bh_find_neighbors: more than 2^31 - 1 neighbours in all: ask in batches";
            return BH_E_INVALID;
        }
        if (outgrown(e->nbr_list_cap, e->nbr_idx, q.total)) {
            TRY(dev_alloc(e, e->nbr_idx, 2 * (size_t)q.total));
            TRY(dev_alloc(e, e->nbr_list, (size_t)q.total));
            e->nbr_list_cap = q.total;
        }
        uint32_t *raw = e->nbr_idx, *sorted = raw + e->nbr_list_cap;
        neighbors_fill(nodes, node_cap, d_T, cidx, px, py, pr, q.r, order, P, rc, pl.offsets, raw,
                       e->stream);
        HIPCHK(e, hipGetLastError());
        int bits = 1;  // caller indices are below the list's size
        while (((int64_t)1 << bits) < e->n) ++bits;
        size_t need = 0;
        HIPCHK(e, neighbors_sort(q.total, P, pl.offsets, raw, sorted, bits, e->nbr_list, nullptr,
                                 need, e->stream));
        if (need > e->nbr_sort_bytes || !e->nbr_sort) {
            if (e->nbr_sort) (void)hipFree(e->nbr_sort);
            e->nbr_sort = nullptr;
            e->nbr_sort_bytes = 0;
            HIPCHK(e, hipMalloc(&e->nbr_sort, need));
            e->nbr_sort_bytes = need;
        }
        size_t have = e->nbr_sort_bytes;
        HIPCHK(e, neighbors_sort(q.total, P, pl.offsets, raw, sorted, bits, e->nbr_list,
                                 e->nbr_sort, have, e->stream));
    }
    q.filled = q.lists && q.total <= q.cap;
    return e->nbr_sw.stop(e, e->stream);
}

// The caller's arguments of bh_find_knn (host arrays) or bh_find_knn_bodies (self: the probes are
// the bodies of the state, nothing is uploaded), and which result planes are wanted.
struct KnnQuery {
    int64_t n;  // probes (self: filled in by the launch, e->n)
    const double *px, *py;
    int k;
    double r_max;
    bool self;
    bool want_idx, want_d2, want_found;
};

// bh_find_knn / bh_find_knn_bodies: the leaf sequence, then -- for a probe list -- upload, key and
// sort as bh_compute_field does, then the seed kernel and the walk into the engine's own planes.
// The bodies are their own probes in slot order, which a full build left in Morton order.
int knn_launch(bh_engine *e, KnnQuery &q, bool tree) {
    if (q.self) q.n = e->n;
    const int64_t P = q.n;
    if (P <= 0) return BH_OK;
    if (tree) TRY(build_leaf_list(e));
    const double *px = e->st.x, *py = e->st.y;
    const uint32_t *map = e->st.cidx;
    if (!q.self) {
        if (outgrown(e->knn_cap, e->knn_in, P)) {
            const size_t cap = (size_t)P;
            TRY(dev_alloc(e, e->knn_in, 2 * cap));   // px, py
            TRY(dev_alloc(e, e->knn_u32, 4 * cap));  // key, sorted key, index, order
            if (e->knn_scratch) (void)hipFree(e->knn_scratch);
            e->knn_scratch = nullptr;
            e->knn_scratch_bytes = field_sort_bytes(P);
            HIPCHK(e, hipMalloc(&e->knn_scratch, e->knn_scratch_bytes ? e->knn_scratch_bytes : 1));
            e->knn_cap = P;
        }
        const size_t cap = (size_t)e->knn_cap;
        double *dx = e->knn_in, *dy = dx + cap;
        TRY(upload_probes(e, Probes{P, q.px, q.py, nullptr}, dx, dy, nullptr));
        uint32_t *key = e->knn_u32, *key_s = key + cap, *idx = key_s + cap, *order = idx + cap;
        HIPCHK(e, field_order(P, dx, dy, e->geo, key, key_s, idx, order, e->knn_scratch,
                              e->knn_scratch_bytes, e->stream));
        px = dx;
        py = dy;
        map = order;
    }
    if (outgrown(e->knn_lane_cap, e->knn_seed, P)) {
        TRY(dev_alloc(e, e->knn_seed, (size_t)P));
        TRY(dev_alloc(e, e->knn_found, (size_t)P));
        e->knn_lane_cap = P;
    }
    const int64_t rows = P * q.k;
    if (outgrown(e->knn_row_cap, e->knn_idx, rows)) {
        TRY(dev_alloc(e, e->knn_idx, (size_t)rows));
        TRY(dev_alloc(e, e->knn_d2, (size_t)rows));
        e->knn_row_cap = rows;
    }
    TRY(e->knn_sw.start(e, e->stream));
    knn_walk(tree ? e->nodes : nullptr, tree ? e->node_cap : 0, tree ? e->base + e->n : nullptr,
             tree ? e->st.cidx : nullptr, tree ? e->leaves : LeafList{nullptr},
             tree ? e->leaf_count : nullptr, map, px, py, q.self, P, q.k, q.r_max, e->geo,
             neighbor_reach_terms(e->geo), e->knn_seed, q.want_idx ? e->knn_idx : nullptr,
             q.want_d2 ? e->knn_d2 : nullptr, q.want_found ? e->knn_found : nullptr, e->stream);
    HIPCHK(e, hipGetLastError());
    return e->knn_sw.stop(e, e->stream);
}

// The planes of bh_find_groups' buffers for the engine's grp_cap.
GroupBufs group_bufs(const bh_engine *e) {
    const size_t cap = (size_t)e->grp_cap, cap1 = cap + 1;
    GroupBufs B{};
    uint32_t *u = e->grp_u32;
    B.parent = u;
    B.minc = u + cap;
    B.rootof = u + 2 * cap;
    B.val = u + 3 * cap;
    B.val_s = u + 4 * cap;
    u += 5 * cap;
    B.flag = u;
    B.gid = u + cap1;
    B.first = u + 2 * cap1;
    B.keep = u + 3 * cap1;
    B.kidx = u + 4 * cap1;
    B.key = e->grp_u64;
    B.key_s = e->grp_u64 + cap;
    B.label = e->grp_i64;
    B.members = e->grp_i64 + cap;
    B.summary = e->grp_i64 + 2 * cap;
    B.part = e->grp_part;
    B.groups = e->grp_groups;
    B.scratch = e->grp_scratch;
    B.scratch_bytes = e->grp_scratch_bytes;
    return B;
}

// bh_find_groups on the tree ensure_tree() left: the leaf sequence, the velocities in this
// build's slot order (a carried tree may have left them in the previous one), then the link walk
// and the catalogue into the engine's own planes and the summary back to the host.  The host
// reads nothing before the walk: lanes beyond the device-side leaf count idle.
int groups_launch(bh_engine *e, double link, int64_t min_members, bh_groups_summary &sum) {
    const int64_t n = e->n;
    TRY(build_leaf_list(e));
    TRY(materialize_velocities(e));
    if (outgrown(e->grp_cap, e->grp_u32, n)) {
        const size_t cap = (size_t)n;
        TRY(dev_alloc(e, e->grp_u32, 10 * cap + 5));
        TRY(dev_alloc(e, e->grp_u64, 2 * cap));
        TRY(dev_alloc(e, e->grp_i64, 2 * cap + 6));
        TRY(dev_alloc(e, e->grp_part, 5 * groups_partial_slots(n)));
        TRY(dev_alloc(e, e->grp_groups, cap));
        if (e->grp_scratch) (void)hipFree(e->grp_scratch);
        e->grp_scratch = nullptr;
        e->grp_scratch_bytes = groups_scratch_bytes(n);
        HIPCHK(e, hipMalloc(&e->grp_scratch, e->grp_scratch_bytes ? e->grp_scratch_bytes : 1));
        e->grp_cap = n;
    }
    // (the planes are laid out for grp_cap; the kernels run over the first n entries of each)
    const GroupBufs B = group_bufs(e);
    groups_prepare(n, B, e->stream);
    HIPCHK(e, hipGetLastError());
    TRY(e->grp_sw_run.start(e, e->stream));
    HIPCHK(e, groups_run(e->nodes, e->node_cap, e->base + n, e->st.cidx, e->leaves, e->leaf_count,
                         e->st.vx, e->st.vy, n, link, min_members, neighbor_reach_terms(e->geo), B,
                         e->stream));
    TRY(e->grp_sw_run.stop(e, e->stream));
    int64_t h[6];
    HIPCHK(e, hipMemcpyAsync(h, B.summary, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    SYNC(e, e->stream);
    sum = bh_groups_summary{h[0], h[1], h[2], h[3], h[4], h[5]};
    if (sum.n_in_tree > 0) std::swap(e->grp_sw, e->grp_sw_run);  // an empty S leaves the reading
    return BH_OK;
}

int evaluate(bh_engine *e, uint32_t *visits, KickMode kick = KICK_NONE, bool *fused = nullptr,
             bool allow_let = false, bool *let_used = nullptr) {
    if (fused) *fused = false;
    if (let_used) *let_used = false;
    // (the pieces are ranges of the slot order: spatially compact only once a full build has
    // put the state into Morton order -- after a reset it is the caller's order)
    if (allow_let && !visits && (e->comm || e->group || e->solo) && let_active(e) &&
        !theta2_is_zero(e) &&
        e->st_morton && e->let_age < BH_LET_REFRESH) {
        bool done = false;
        TRY(evaluate_let(e, kick, &done));
        if (done) {
            ++e->let_age;
            if (let_used) *let_used = true;
            if (fused) *fused = true;  // integrated in the evaluation
            return BH_OK;
        }
    }
    TRY(ensure_tree(e));
    const int64_t n = e->n;
    ForceParams fp = force_params(e);  // BHA:378
    const uint32_t *d_T = e->base + n;
    const bool direct = fp.theta2 == 0.0 && !visits;
    if (direct) TRY(build_leaf_list(e));
    const TraverseCounters counters{visits, e->contrib32, e->wave_iters, e->wave_blocks};
    const uint32_t *lanes = e->lanes_valid ? e->lanes : nullptr;  // [lo, hi): lane ranges
    e->a2_lanes = direct ? nullptr : lanes;
    e->a2_layout = GatherLayout{};
    auto forces = [&](int64_t lo, int64_t hi, uint32_t *vis, hipStream_t fs, double *a2) {
        if (direct)
            direct_forces(e->leaves, e->leaf_count, e->st.x, e->st.y, e->st.m, lo, hi, fp.G,
                          fp.soft2, a2, fs);
        else
            traverse(e->nodes, e->node_cap, d_T, e->st.x, e->st.y, e->st.m, e->st.cidx, lo, hi, e->geo, fp,
                     a2, vis ? &counters : nullptr, fs, nullptr, lanes);
    };
    if ((!e->comm && !e->group && !e->solo) || visits) {
        if (kick != KICK_NONE && !direct && !visits && fused) {
            KickArgs ka{kick, e->st.vx, e->st.vy, e->p.dt * 0.5, e->p.dt};
            if (e->vel_perm && kick == KICK_DRIFT) {  // v[p] = old v[perm[p]]
                ka.svx = e->alt.vx;
                ka.svy = e->alt.vy;
                ka.perm = e->vel_perm;
                e->vel_perm = nullptr;
            }
            TRY(materialize_velocities(e));  // (any other path: permuted first)
            // (not into a breadth-first walk: one body per wave would make one bucket-count
            // atomic per body -- C1 'R' 37.6 against 21.2 us for the kick-only walk --, the build's
            // k_morton_count aggregates them per wave)
            if (e->fuse_keys && kick == KICK_DRIFT && e->spl_nb > 0 && n > 0 &&
                !traverse_is_bfs(e->node_cap, 0, n, KICK_DRIFT, false)) {
                ka.mf = MortonFuse{e->keys, e->keys32, e->spl, e->spl_nb, e->cnt, e->base,
                                   e->bcount};
                e->keys_ready = true;
            }
            e->fuse_keys = false;
            WaveOrder wo;
            TRY(wave_order_for(e, 0, n, e->stream, wo));
            traverse(e->nodes, e->node_cap, d_T, e->st.x, e->st.y, e->st.m, e->st.cidx, 0, n, e->geo, fp,
                     e->a2, nullptr, e->stream, &ka, lanes, &wo);
            *fused = true;
            HIPCHK(e, hipGetLastError());
            TRY(mark(e, 1));
            return wave_order_next(e, 0, n, e->stream);
        } else {
            forces(0, n, visits, e->stream, e->a2);
        }
        HIPCHK(e, hipGetLastError());
        TRY(mark(e, 1));
        return BH_OK;
    }
    const int64_t sub = shard_sub(n, e->world, BH_SHARD_ROUNDS);
    if (e->solo)  // measurement: the peers' bodies get no force
        HIPCHK(e, hipMemsetAsync(e->a2, 0, sizeof(double) * 2 * (size_t)(sub * e->world *
                                                                         BH_SHARD_ROUNDS),
                                 e->stream));
    if (e->group) {  // a collective's implicit ordering: peers' copies of our last pieces done
        TRY(group_barrier(e));
        for (bh_engine *peer : e->group->members)
            if (peer != e) HIPCHK(e, hipStreamWaitEvent(e->stream, peer->gathered_ev, 0));
    }
    TRY(round_streams(e));
    const GatherLayout gl = shard_layout(n, e->world);
    e->a2_layout = gl;
    for (int k = 0; k < BH_SHARD_ROUNDS; ++k) {
        int64_t lo = 0, hi = 0;
        bh_shard_range(n, e->rank, e->world, k, &lo, &hi);
        hipStream_t rs = (k & 1) ? e->stream2 : e->stream;
        forces(lo, hi, nullptr, rs, e->a2 + 2 * (gather_slot(gl, lo) - lo));
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->round_ev[k], rs));
        HIPCHK(e, hipStreamWaitEvent(e->comm_stream, e->round_ev[k], 0));
        if (e->group) TRY(group_barrier(e));  // every member recorded round k
        TRY(gather_round(e, gl, k, 2, k, COLL_ACC));
    }
    TRY(mark(e, 1));
    HIPCHK(e, hipEventRecord(e->gathered_ev, e->comm_stream));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->gathered_ev, 0));
    TRY(mark(e, 4));
    return BH_OK;
}

int check_tree_flags(bh_engine *e) {
    uint32_t flags = 0;
    HIPCHK(e, hipMemcpyAsync(&flags, e->scalars + 1, sizeof(uint32_t), hipMemcpyDeviceToHost,
                             e->stream));
    SYNC(e, e->stream);
    if (flags) {
        e->err = "jitter replay reached an unsupported geometry (body stayed inside a depth J+1 cell)";
        return BH_E_STATE;
    }
    return BH_OK;
}

// The frame of a call that evaluates on the full tree without stepping (bh_compute_*), on one
// engine.  query_begin: the call is counted, the device current, the phase marks and the tree
// flags cleared.  Between the two the call enqueues on e->stream: ensure_tree() or evaluate()
// unless there are no bodies, then its own kernels.  query_end, had_tree: the tree's jitter is in
// the state (the mirror is stale), the stream is waited for and the build's flags are checked --
// only then may results be copied out; either way the phase timings are collected.
int query_begin(bh_engine *e) {
    e->prog_api.store(++e->api_calls);
    HIPCHK(e, hipSetDevice(e->device));
    e->ev_used = 0;
    e->timings_pending = false;
    HIPCHK(e, hipMemsetAsync(e->scalars + 1, 0, sizeof(uint32_t), e->stream));
    return BH_OK;
}

int query_end(bh_engine *e, bool had_tree) {
    if (had_tree) {
        e->mir_fresh = false;
        SYNC(e, e->stream);
        TRY(check_tree_flags(e));
    }
    if (e->profiling) TRY(collect_timings(e));
    return BH_OK;
}

// ---- merge rule (BHA:463-532) ---------------------------------------------------------
// Entirely on the device, no host round trip: heavy bodies (m > mergeMaxMass) and every
// (heavy, body) pair closer than mergeMinDist are collected in parallel, then one workgroup
// replays the reference's sequential rule over the pairs sorted by caller index
// (integrate.hip k_merge_replay).  Removed bodies become tombstones that leave the tree, the
// candidate search and the output at once; the state is compacted once per bh_step call
// (finish_merges).  Heavy bodies only gain mass and never appear, so once a call ends with
// none the rule is skipped until the bodies or mergeMaxMass change.
int pinned_reserve(bh_engine *e, size_t bytes) {
    if (bytes <= e->pin_bytes) return BH_OK;
    if (e->pin) (void)hipHostFree(e->pin);
    e->pin = nullptr;
    size_t nb = std::max<size_t>(bytes, 1 << 16);
    // coherent: kernels write their small results here directly (finish_merges' read-back)
    HIPCHK(e, hipHostMalloc(&e->pin, nb, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(e, hipHostGetDevicePointer(&e->pin_dev, e->pin, 0));
    e->pin_bytes = nb;
    return BH_OK;
}

int merge_bufs(bh_engine *e) {
    // two candidate pairs per body, or what an overflowing step needed (bh_step's retry)
    const uint32_t cap = (uint32_t)std::min<int64_t>(
        0xFFFFFFF0ll, std::max<int64_t>({1 << 16, 2 * e->cap, (int64_t)e->box_need}));
    if (!e->box || e->box_cap < cap) {
        e->box_cap = cap;
        TRY(dev_alloc(e, e->box, (size_t)cap + 1));
        TRY(dev_alloc(e, e->rkeys, 2 * (size_t)cap));
        TRY(dev_alloc(e, e->ridx, 2 * (size_t)cap));
    }
    if (e->dlog_cap < e->cap) {  // at most every body is removed within one call
        TRY(dev_alloc(e, e->dlog, (size_t)e->cap + 1));
        TRY(dev_alloc(e, e->dead_sorted, (size_t)e->cap + 1));
        TRY(dev_alloc(e, e->mbits, ((size_t)e->cap >> 5) + 2));
        TRY(dev_alloc(e, e->mslot, (size_t)e->cap + 1));
        e->dlog_cap = e->cap;
    }
    return BH_OK;
}

// s: the engine's stream, or pipe_stream in the pipelined step (no phase marks there)
// header_zeroed: the caller cleared the mailbox header on an earlier stream position (the
// pipelined step does it before the second traversal, where a fill kernel is not starved)
int merge(bh_engine *e, hipStream_t s = nullptr, bool header_zeroed = false) {
    if (e->p.merge_min_dist <= 0.0 || e->n <= 1 || !e->heavy_possible) return BH_OK;  // BHA:465
    const bool marks = !s;
    if (!s) s = e->stream;
    TRY(materialize_positions(e));
    if (marks) TRY(mark(e, -1));
    TRY(merge_bufs(e));
    const double minD2 = e->p.merge_min_dist * e->p.merge_min_dist;  // BHA:468
    uint32_t *hc = e->heavy_ready ? e->scalars + 14 : nullptr;  // listed by the last build
    e->heavy_ready = false;
    if (hc) e->heavy_dirty = false;  // (k_merge_replay clears the count)
    merge_candidates(e->n, e->st.x, e->st.y, e->st.m, e->st.cidx, e->p.merge_max_mass, minD2,
                     e->heavy, e->box, e->box_cap, s, header_zeroed, hc);
    merge_replay(e->box, e->box_cap, e->st.m, e->st.cidx, e->scalars, e->dlog, e->rkeys, e->ridx,
                 e->mbits, e->mslot, e->n, s, hc);
    HIPCHK(e, hipGetLastError());
    e->merge_ran = true;
    if (marks) TRY(mark(e, 3));
    return BH_OK;
}

// End of a bh_step call (the stream is idle): read the removal count, compact the state and
// renumber caller indices; record the removals for bh_last_removed.  *overflow receives the
// candidate count of a step whose pairs did not fit the mailbox (nothing is compacted then:
// the call is replayed from its snapshot with a larger mailbox, see bh_step).
// *tree_flags receives scalars[1] (the builds' error flags) when the merge rule ran (the same
// read-back), else *have_flags stays false.
int finish_merges(bh_engine *e, uint32_t *overflow, uint32_t *tree_flags = nullptr,
                  bool *have_flags = nullptr) {
    *overflow = 0;
    e->removed.clear();
    if (!e->merge_ran) return BH_OK;
    e->merge_ran = false;
    TRY(materialize_positions(e));
    // one round trip: the counts, the mailbox header and the first DLOG_AHEAD removals (a step
    // removes tens of bodies at C3) come back together
    constexpr uint32_t DLOG_AHEAD = 4096;
    TRY(pinned_reserve(e, 64 + 2 * sizeof(uint32_t) * DLOG_AHEAD));
    uint32_t *h = static_cast<uint32_t *>(e->pin);
    uint32_t *hlog = h + 16, *hsorted = h + 16 + DLOG_AHEAD;
    // (one kernel writes it all into the pinned buffer: no copies -- four were four blit kernels,
    // and a DMA copy queued behind the mirror's 40 MB on the same engine, round 4 trace)
    const uint32_t ahead = (uint32_t)std::min<int64_t>(DLOG_AHEAD, e->dlog_cap);
    pack_readback(e->scalars, e->box, e->dlog, ahead, static_cast<uint32_t *>(e->pin_dev),
                  e->stream);
    HIPCHK(e, hipGetLastError());
    SYNC(e, e->stream);
    if (tree_flags) *tree_flags = h[1];
    if (have_flags) *have_flags = true;
    const uint32_t nd = h[2];
    const uint32_t nd_before_last = h[12];  // removals before the call's last merge rule
    const MergeHeader hdr = *reinterpret_cast<const MergeHeader *>(h + 4);
    if (h[3]) {
        *overflow = h[3];
        return BH_OK;
    }
    if (hdr.heavies == 0) e->heavy_possible = false;
    if (nd == 0) return BH_OK;
    std::vector<uint32_t> dead(nd);
    if (nd <= ahead) {
        std::memcpy(dead.data(), hlog, 4 * (size_t)nd);
    } else {
        HIPCHK(e, hipMemcpy(dead.data(), e->dlog, 4 * (size_t)nd, hipMemcpyDeviceToHost));
    }
    std::sort(dead.begin(), dead.end());
    if (nd <= DLOG_AHEAD) {  // from pinned memory, in stream order: no wait
        std::memcpy(hsorted, dead.data(), 4 * (size_t)nd);
        HIPCHK(e, hipMemcpyAsync(e->dead_sorted, hsorted, 4 * (size_t)nd, hipMemcpyHostToDevice,
                                 e->stream));
    } else {
        HIPCHK(e, hipMemcpy(e->dead_sorted, dead.data(), 4 * (size_t)nd, hipMemcpyHostToDevice));
    }
    const int64_t n = e->n;
    if (e->view_pending) {  // the caller-visible state (the previous order) loses the same bodies
        HIPCHK(e, compact_state(n, e->keep, e->view, e->alt, e->dead_sorted, nd, e->pos,
                                e->scratch, e->scratch_bytes, e->stream));
        std::swap(e->view, e->alt);
    }
    // (a prebuilt tree stays valid: the removed bodies were tombstones in its build, sentinel keys
    // at the tail of its order, so the compaction moves no slot the tree refers to, and its node
    // count base[n'] is the same for every n' at or past the last body in the tree)
    HIPCHK(e, compact_state(n, e->keep, e->st, e->alt, e->dead_sorted, nd, e->pos, e->scratch,
                            e->scratch_bytes, e->stream));
    std::swap(e->st, e->alt);
    e->boxes_valid = false;  // the slots moved
    if (e->lanes_valid) {  // carry the wave grouping over the removals (no re-sort)
        HIPCHK(e, compact_lanes(n, e->lanes, e->keep, e->pos, e->idx, e->keys32, e->keys32_s,
                                e->scratch, e->scratch_bytes, e->stream));
        std::swap(e->lanes, e->keys32_s);
        e->inv_valid = false;
    }
    e->n = n - (int64_t)nd;
    e->inv_valid = false;  // another n: another exchange layout
    if ((e->comm || e->group || e->solo) && let_active(e) && !theta2_is_zero(e) && e->n > 0 &&
        e->st_morton && !e->pos_pending) {
        // the LET selections until the next full build: boxes of the compacted slots from the
        // positions now (materialized at the call's end), the displacement bound restarting here
        TRY(let_alloc(e, 0));
        let_boxes(e->n, e->st, e->geo, e->let_box, e->stream);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipMemsetAsync(e->disp, 0, sizeof(double), e->stream));
        e->boxes_valid = true;
        e->builds_since_box = 0;
    }
    e->removed.assign(dead.begin(), dead.end());
    // BHA:526: lastTree = null only when the last step's merge rule removed a body.  Bodies
    // removed by earlier steps were tombstones in the last build (sentinel keys: the tail of its
    // order), so its first n - nd sorted keys still describe the whole tree.
    if (nd != nd_before_last) {
        e->tree_valid = false;
        e->lazy_tree = false;
        e->lt_aside = false;
    } else if (e->lazy_tree) {  // the snapshot follows the compaction (its tombstones were not built)
        compact_pair(n, e->keep, e->pos, e->lt_x, e->lt_y, e->alt.x, e->alt.y, e->stream);
        HIPCHK(e, hipGetLastError());
        std::swap(e->lt_x, e->alt.x);
        std::swap(e->lt_y, e->alt.y);
    }
    SYNC(e, e->stream);
    return BH_OK;
}

// ---- tracers (bh_set_tracers) ----------------------------------------------------------
// The lane map of the tracers: their order along the build's Morton curve (field_order, what
// bh_compute_field makes for its probes), on the engine's stream.
int tracer_reorder(bh_engine *e) {
    const size_t n = (size_t)e->trc_n;
    uint32_t *key = e->trc_u32, *key_s = key + n, *idx = key_s + n, *order = idx + n;
    HIPCHK(e, field_order(e->trc_n, e->trc, e->trc + n, e->geo, key, key_s, idx, order,
                          e->trc_scratch, e->trc_scratch_bytes, e->stream));
    e->trc_age = 0;
    return BH_OK;
}

// One evaluation of the tracers on the tree the bodies' traversal of the same evaluation read
// (d_T null: no tree), on the engine's stream right behind it.  A step's first walk re-makes a lane
// map that has served R steps.  No tracers: nothing is launched and no event is recorded.
int tracer_walk(bh_engine *e, const Node *nodes, size_t node_cap, const uint32_t *d_T,
                KickMode kick) {
    const int64_t nt = e->trc_n;
    if (nt <= 0) return BH_OK;
    if (kick == KICK_DRIFT) {
        if (e->trc_age >= (int)tracer_shape(nt).reorder) TRY(tracer_reorder(e));
        ++e->trc_age;
    }
    const size_t s = (size_t)nt;
    TRY(mark(e, PHASE_START));
    tracer_step(nodes, node_cap, d_T, e->trc, e->trc + s, e->trc + 2 * s, e->trc + 3 * s,
                e->trc_u32 + 3 * s, nt, e->geo, force_params(e), kick, e->p.dt * 0.5, e->p.dt,
                e->stream);
    HIPCHK(e, hipGetLastError());
    return mark(e, PHASE_TRACERS);
}

void tracer_free(bh_engine *e) {
    for (void **q : {(void **)&e->trc, (void **)&e->trc_snap, (void **)&e->trc_u32,
                     &e->trc_scratch}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    e->trc_scratch_bytes = 0;
    e->trc_n = e->trc_snap_n = 0;
    e->trc_age = 0;
}

// The tracers at the start of a bh_step call that may be replayed, and back: a replayed call
// steps them exactly once.  (The lane map a discarded attempt re-made is still a permutation of
// the same list; its age is the snapshot's, so a replay re-makes it at the same steps.)
int tracer_snapshot(bh_engine *e) {
    const int64_t nt = e->trc_n;
    if (nt <= 0) return BH_OK;
    if (e->trc_snap_n != nt || !e->trc_snap) {
        e->trc_snap_n = 0;
        TRY(dev_alloc(e, e->trc_snap, 4 * (size_t)nt));
        e->trc_snap_n = nt;
    }
    HIPCHK(e, hipMemcpyAsync(e->trc_snap, e->trc, sizeof(double) * 4 * (size_t)nt,
                             hipMemcpyDeviceToDevice, e->stream));
    e->trc_snap_age = e->trc_age;
    return BH_OK;
}

int tracer_restore(bh_engine *e) {
    const int64_t nt = e->trc_n;
    if (nt <= 0) return BH_OK;
    if (e->trc_snap_n != nt) {
        e->err = "tracers: a replayed call has no snapshot of the tracer list";
        return BH_E_STATE;
    }
    HIPCHK(e, hipMemcpyAsync(e->trc, e->trc_snap, sizeof(double) * 4 * (size_t)nt,
                             hipMemcpyDeviceToDevice, e->stream));
    e->trc_age = e->trc_snap_age;
    return BH_OK;
}

// ---- the step log (bh_set_step_log) ------------------------------------------------------
void step_log_free(bh_engine *e, bool ring) {
    for (void **q : {(void **)&e->slog_phi, (void **)&e->slog_stage, (void **)&e->slog_part,
                     (void **)&e->slog_keep, (void **)&e->slog_pos, &e->slog_tmp}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    e->slog_tmp_bytes = 0;
    e->slog_bcap = 0;
    e->slog_phi_valid = false;
    if (ring) {
        if (e->slog_ring) (void)hipFree(e->slog_ring);
        e->slog_ring = nullptr;
        e->slog_cap = 0;
    }
}

// The log's per-body buffers for the engine's body capacity (before a call's first step).
int step_log_bufs(bh_engine *e) {
    if (e->slog_cap <= 0 || (e->slog_bcap >= e->cap && e->slog_part)) return BH_OK;
    step_log_free(e, false);
    const size_t c = (size_t)std::max<int64_t>(e->cap, 1);
    TRY(dev_alloc(e, e->slog_phi, c));
    TRY(dev_alloc(e, e->slog_stage, 6 * c));
    TRY(dev_alloc(e, e->slog_keep, c));
    TRY(dev_alloc(e, e->slog_pos, c));
    TRY(dev_alloc(e, e->slog_part, diag_partial_doubles()));
    e->slog_tmp_bytes = compact_scratch_bytes((int64_t)c);
    HIPCHK(e, hipMalloc(&e->slog_tmp, e->slog_tmp_bytes ? e->slog_tmp_bytes : 1));
    e->slog_bcap = (int64_t)c;
    return BH_OK;
}

// One step's record, enqueued on the engine's stream behind the step's second kick: e->slog_phi
// holds the potential of every slot on the tree that evaluation walked; cidx and m are the flags
// and masses that evaluation read (before the step's merge rule).  The bodies of the step's list
// -- the slots without a tombstone, by caller index -- go to the log's planes in list order and
// are reduced there; the record lands in the ring's next slot.  No host wait, no host copy.
int step_log_step(bh_engine *e, const uint32_t *cidx, const double *m) {
    if (e->slog_cap <= 0) return BH_OK;
    const int64_t n = e->n, c = e->slog_bcap;
    hipStream_t s = e->stream;
    TRY(mark(e, PHASE_START));
    if (n > 0) {
        HIPCHK(e, mirror_index(n, cidx, e->slog_keep, e->slog_pos, e->slog_tmp, e->slog_tmp_bytes,
                               s));
        double *st = e->slog_stage;
        const double *s5[5] = {e->st.x, e->st.y, e->st.vx, e->st.vy, m};
        double *d5[5] = {st, st + c, st + 2 * c, st + 3 * c, st + 4 * c};
        mirror_scatter(n, cidx, e->slog_pos, 5, s5, d5, s);
        const double *s1[1] = {e->slog_phi};
        double *d1[1] = {st + 5 * c};
        mirror_scatter(n, cidx, e->slog_pos, 1, s1, d1, s);
    }
    e->slog_step += 1;
    e->slog_t += e->p.dt;
    char *slot = static_cast<char *>(e->slog_ring) +
                 sizeof(bh_step_record) * (size_t)(e->slog_head % e->slog_cap);
    e->slog_head += 1;
    step_log_record(n, e->slog_keep, e->slog_pos, e->slog_stage, c, e->slog_part, e->slog_step,
                    e->slog_t, slot, s);
    HIPCHK(e, hipGetLastError());
    e->slog_phi_valid = true;
    return mark(e, PHASE_STEP_LOG);
}

// Copy of the state at the start of a bh_step call that may merge: if a step's candidate
// pairs overflow the mailbox, the call is replayed from here with a larger one, so the rule
// (BHA:478-520) holds for any number of pairs.
int copy_state(bh_engine *e, const BodyState &src, const BodyState &dst, int64_t n) {
    if (n <= 0) return BH_OK;
    const size_t d = sizeof(double) * (size_t)n;
    HIPCHK(e, hipMemcpyAsync(dst.x, src.x, d, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst.y, src.y, d, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst.vx, src.vx, d, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst.vy, src.vy, d, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst.m, src.m, d, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst.cidx, src.cidx, sizeof(uint32_t) * (size_t)n,
                             hipMemcpyDeviceToDevice, e->stream));
    return BH_OK;
}

int snapshot(bh_engine *e) {
    TRY(materialize_positions(e));
    if (e->snap_cap < e->cap) {
        TRY(alloc_state(e, e->snap, (size_t)e->cap));
        e->snap_cap = e->cap;
    }
    e->snap_n = e->n;
    TRY(tracer_snapshot(e));
    // after a pipelined call the caller's state is the view (the prebuilt tree's jitter is not
    // applied yet): a replay starts from it and builds its own first tree.  The call never writes
    // the view's buffers (its own last step makes a new view from `alt`), so the snapshot takes
    // them over instead of copying 44 B per body
    if (e->view_pending && e->view_cap == e->snap_cap) {
        std::swap(e->snap, e->view);
        return BH_OK;
    }
    return copy_state(e, e->view_pending ? e->view : e->st, e->snap, e->n);
}

int restore(bh_engine *e) {
    e->vel_perm = nullptr;  // (the snapshot is complete)
    TRY(copy_state(e, e->snap, e->st, e->snap_n));
    TRY(tracer_restore(e));
    e->slog_head = e->slog_call_head;  // a replayed call logs each step once
    e->slog_step = e->slog_call_step;
    e->slog_t = e->slog_call_t;
    e->n = e->snap_n;
    TRY(drop_carried_flags(e));
    e->prebuilt = false;
    e->view_pending = false;
    e->lt_aside = false;
    e->mir_fresh = false;
    e->spl_nb = 0;  // the splitters describe the discarded builds' order
    e->keys_ready = false;
    e->lanes_valid = e->lr_pending = e->lr_ready = false;
    e->inv_valid = false;
    e->pos_pending = false;  // the snapshot holds every position
    e->boxes_valid = false;
    e->heavy_possible = true;
    e->tree_valid = false;
    e->st_morton = false;
    e->vel_stale = false;  // the snapshot is a consistent replica
    return BH_OK;
}

// End of a bh_step call with LET builds (every rank's stream is idle): the call's LET status words
// scalars[4] (some subset overflowed, or a rank-local guard fired) and scalars[5] (largest subset),
// max-reduced over the ranks, so that every rank replays the call or none does.
int agree_let_flags(bh_engine *e, uint32_t ls[2], uint32_t *own_sub) {
    HIPCHK(e, hipMemcpy(ls, e->scalars + 4, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *own_sub = ls[1];
    if (!e->solo) TRY(coll_log(e, COLL_FLAGS, 2 * sizeof(uint32_t), CS_MAIN));
    if (e->comm) {
        NCCLCHK(e, ncclAllReduce(e->scalars + 4, e->scalars + 4, 2, ncclUint32, ncclMax, e->comm,
                                 e->stream));
        HIPCHK(e, hipMemcpyAsync(ls, e->scalars + 4, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                 e->stream));
        SYNC(e, e->stream);
        return BH_OK;
    }
    if (!e->group) return BH_OK;  // solo: no peers
    // a member that cannot read a peer's flags must not decide alone: every member sees its
    // failure after the second barrier and all return an error together (none replays)
    e->agree_failed = false;  // (its previous value was read before this call's LET barriers)
    TRY(group_barrier(e));      // every member's call is complete on the device
    for (bh_engine *peer : e->group->members) {
        if (peer == e) continue;
        uint32_t q[2] = {0, 0};
        const hipError_t rc = hipMemcpy(q, peer->scalars + 4, sizeof(q), hipMemcpyDeviceToHost);
        if (rc != hipSuccess) {
            e->agree_failed = true;
            e->err = std::string("agree_let_flags: ") + hipGetErrorString(rc);
            break;
        }
        ls[0] = std::max(ls[0], q[0]);
        ls[1] = std::max(ls[1], q[1]);
    }
    TRY(group_barrier(e));  // nobody clears its flags (a replay) before every member has read them
    bool failed = false;
    for (bh_engine *peer : e->group->members) failed = failed || peer->agree_failed;
    if (failed) {
        if (!e->agree_failed) e->err = "agree_let_flags: a peer could not read the LET flags";
        return BH_E_DEVICE;
    }
    return BH_OK;
}

// ---- the pipelined step (one GPU) -----------------------------------------------------
// Step s's second traversal (a(t+dt), BHA:421-433) and step s+1's first build (BHA:359, over the
// same positions after the merge rule, BHA:438) are independent: the kick writes only
// velocities, the merge rule only masses and flags, and the build reads neither velocities nor
// the traversal's output.  So the merge rule and the next build run on a second stream while the
// traversal runs -- the build kernels (single-workgroup span passes, scans, sorts: ~260 us of
// mostly under-filled launches per build at C3) fill the chip next to the traversal's tail.
// The traversal reads copies of what they overwrite (masses, flags, lane map, node count) and
// the build writes the other node array; the velocities follow the build's permutation once
// the kick is done.  Every kernel sees the inputs of the sequential order: bit-identical.
// The pipeline stops at the next build: the next step's a(t) evaluated beside this step's second
// traversal as well was measured slower at C3 (1.925 against 1.884 ms per step, round 4,
// DESIGN.md) -- the next tree is ready only after the traversal's last waves are placed, so the
// two evaluations barely overlap and share the caches when they do.
// A call's last step is pipelined too (the next call starts on its tree).
bool pipelined(const bh_engine *e) {
    return e->n > 0 && !e->comm && !e->group && !e->solo && !theta2_is_zero(e);
}

// The overlap and mirror streams of a one-GPU engine.  HIP hands a process's streams its few
// hardware queues (GPU_MAX_HW_QUEUES = 4) in creation order, so bh_create makes the overlap
// stream right after the engine's own, and a caller that reads the mirror enables it right after
// bh_create: made later, after another engine's streams (bench.py's counter probe), the mirror's
// copies shared a queue with the step's kernels (C3 one-step calls with the mirror: 3.25 -> 2.3
// ms).  An engine that never enables the mirror holds two queues, not three.
// The exchange stream (RCCL all-gathers, or the in-process copies) at the high priority: its
// few workgroups are dispatched ahead of the traversal rounds' queued ones as soon as a slot
// frees, instead of in the last round's tail
hipError_t comm_stream_create(hipStream_t *s) {
    int lo = 0, hi = 0;
    hipError_t rc = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (rc != hipSuccess) return rc;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi);
}

// The pipelined step's cross-stream events order work on this device only: no system-scope fence
// when they are recorded (the default one writes back and invalidates the caches for the host)
constexpr unsigned kPipeEvFlags = hipEventDisableTiming | hipEventDisableSystemFence;
int pipe_streams(bh_engine *e) {
    for (hipEvent_t &ev : e->pipe_ev)
        if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, kPipeEvFlags));
    if (!e->pipe_stream) {
        // the traversal fills every wave slot with a queue of waiting workgroups: at the default
        // priority the overlapped kernels would be dispatched only in its tail
        int lo = 0, hi = 0;
        HIPCHK(e, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(e, hipStreamCreateWithPriority(&e->pipe_stream, hipStreamNonBlocking, hi));
    }
    return BH_OK;
}

int mirror_streams(bh_engine *e) {
    if (!e->mir_stream) {
        int lo = 0, hi = 0;
        HIPCHK(e, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(e, hipStreamCreateWithPriority(&e->mir_stream, hipStreamNonBlocking, hi));
        for (hipEvent_t *ev : {&e->mir_ev, &e->mir_ev2, &e->mir_ev3, &e->mir_in[0], &e->mir_in[1],
                               &e->mid_ev, &e->mid_sv_ev})
            HIPCHK(e, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    return BH_OK;
}

int pipe_alloc(bh_engine *e, bool last) {
    if (e->nodes_alt_cap < e->node_cap) {
        TRY(dev_alloc(e, e->nodes_alt, e->node_cap));
        e->nodes_alt_cap = e->node_cap;
    }
    if (last && e->view_cap < e->cap) {
        TRY(alloc_state(e, e->view, (size_t)e->cap));
        e->view_cap = e->cap;
    }
    if (last && e->lt_walk_cap < e->cap) {
        TRY(dev_alloc(e, e->lt_keys, (size_t)e->cap));
        TRY(dev_alloc(e, e->lt_cpl, (size_t)e->cap + 32));  // (as cpl: they trade places)
        TRY(dev_alloc(e, e->lt_base, (size_t)e->cap + 1));
        e->lt_walk_cap = e->cap;
    }
    if (e->trav_cap < e->cap) {
        TRY(dev_alloc(e, e->m_trav, (size_t)e->cap));
        TRY(dev_alloc(e, e->cidx_trav, (size_t)e->cap));
        TRY(dev_alloc(e, e->lanes_trav, (size_t)e->cap));
        if (!e->T_trav) TRY(dev_alloc(e, e->T_trav, 1));
        e->trav_cap = e->cap;
    }
    return pipe_streams(e);
}

// ---- the pinned caller-order mirror (bh_set_mirror / bh_map_bodies) -------------------
// The front-end reads every body after every step (PNL:302-306).  With the mirror on, a call's
// last step writes the bodies in the caller's order (after the call's removals, BHA:519) into
// pinned host memory itself: positions and masses as soon as the merge rule is done, velocities
// when the last traversal's kick is -- the device-to-host copies run on the DMA engines while the
// overlapped next build (and the traversal's tail) still run.
int mirror_alloc(bh_engine *e) {
    if (e->mir_cap < e->cap || (e->mir_nbuf == 2 && !e->mir_buf[1])) {
        for (double *&b : e->mir_buf) {
            if (b) (void)hipHostFree(b);
            b = nullptr;
        }
        e->mir = nullptr;
        e->mir_cap = 0;
        e->mir_front = -1;
        for (int i = 0; i < e->mir_nbuf; ++i)
            HIPCHK(e, hipHostMalloc((void **)&e->mir_buf[i], sizeof(double) * 5 * (size_t)e->cap,
                                    hipHostMallocDefault));
        e->mir = e->mir_buf[0];
        if (e->mir_idx) (void)hipHostFree(e->mir_idx);
        e->mir_idx = nullptr;
        if (e->mir_nbuf == 2) {  // the survivors' list indices for bh_step_positions
            const size_t w = MIRROR_HDR + (size_t)e->cap;
            HIPCHK(e, hipHostMalloc((void **)&e->mir_idx, sizeof(uint32_t) * w, hipHostMallocDefault));
            TRY(dev_alloc(e, e->mir_idx_stage, w));
        }
        TRY(dev_alloc(e, e->mir_stage, 5 * (size_t)e->cap));
        TRY(dev_alloc(e, e->mir_keep, (size_t)e->cap));
        TRY(dev_alloc(e, e->mir_pos, (size_t)e->cap));
        const size_t tb = compact_scratch_bytes(e->cap);
        if (e->mir_tmp) (void)hipFree(e->mir_tmp);
        e->mir_tmp = nullptr;
        HIPCHK(e, hipMalloc(&e->mir_tmp, tb));
        e->mir_tmp_bytes = tb;
        e->mir_cap = e->cap;
        e->mir_fresh = false;
    }
    return mirror_streams(e);
}

// src: the state the caller sees (tombstones of the running call still in it); its positions,
// masses and caller indices are final once after_pos's queued work is, its velocities once
// after_vel's is.  e->n bodies (before the call's compaction).
// The velocities are gathered on after_vel itself, right behind their producer: queued on the
// mirror stream they waited for the positions' host copies (~0.35 ms in the one-step call,
// which waits for them before its compaction -- round 4 drop-in trace).  (Kernels storing
// straight into coherent pinned memory instead of the staging copies measured slower: one-step
// calls with the mirror 3.33 against 3.20 ms.)
// (in two parts, so that the positions can be queued before the work after_vel still gets)
// in_line: the index and the gather run on after_pos itself, only the copies on the mirror
// stream (before a traversal: queued beside it they wait for its first waves to retire)
int mirror_pos(bh_engine *e, const BodyState &src, hipStream_t after_pos, bool in_line = false) {
    TRY(mirror_alloc(e));
    if (e->mir_nbuf == 2 && e->mir_buf[1])  // never the buffer the caller holds
        e->mir = e->mir_buf[e->mir_front == 0 ? 1 : 0];
    const int64_t n = e->n;
    const int64_t c = e->mir_cap;
    hipStream_t ms = e->mir_stream;
    hipStream_t ws = in_line ? after_pos : ms;
    if (!in_line) {
        HIPCHK(e, hipEventRecord(e->mir_in[0], after_pos));
        HIPCHK(e, hipStreamWaitEvent(ms, e->mir_in[0], 0));
    }
    if (n > 0) {
        double *st = e->mir_stage;
        HIPCHK(e, mirror_index(n, src.cidx, e->mir_keep, e->mir_pos, e->mir_tmp, e->mir_tmp_bytes,
                               ws));
        HIPCHK(e, hipEventRecord(e->mir_in[1], ws));  // the caller positions are known
        const double *s3[3] = {src.x, src.y, src.m};
        double *d3[3] = {st, st + c, st + 4 * c};
        mirror_scatter(n, src.cidx, e->mir_pos, 3, s3, d3, ws);
        HIPCHK(e, hipGetLastError());
        if (e->mir_idx) {  // two buffers: the survivors' indices in the list before the call
            mirror_survivors(n, e->mir_keep, e->mir_pos, e->scalars, e->mir_idx_stage, ws);
            HIPCHK(e, hipGetLastError());
        }
        HIPCHK(e, hipEventRecord(e->mir_ev3, ws));  // the positions' gather is done
        if (in_line) HIPCHK(e, hipStreamWaitEvent(ms, e->mir_ev3, 0));
        if (e->mir_idx) {  // first: the caller's removal pass needs only them (bh_step_positions)
            HIPCHK(e, hipMemcpyAsync(e->mir_idx, e->mir_idx_stage,
                                     sizeof(uint32_t) * (MIRROR_HDR + (size_t)n),
                                     hipMemcpyDeviceToHost, ms));
            HIPCHK(e, hipEventRecord(e->mid_sv_ev, ms));
        }
        for (int j : {0, 1, 4})  // (the survivors are a prefix of each array)
            HIPCHK(e, hipMemcpyAsync(e->mir + j * c, st + j * c, sizeof(double) * n,
                                     hipMemcpyDeviceToHost, ms));
    }
    return BH_OK;
}

int mirror_vel(bh_engine *e, const BodyState &src, hipStream_t after_vel) {
    const int64_t n = e->n;
    const int64_t c = e->mir_cap;
    hipStream_t ms = e->mir_stream;
    if (n > 0) {
        double *st = e->mir_stage;
        HIPCHK(e, hipStreamWaitEvent(after_vel, e->mir_in[1], 0));
        const double *s2[2] = {src.vx, src.vy};
        double *d2[2] = {st + 2 * c, st + 3 * c};
        mirror_scatter(n, src.cidx, e->mir_pos, 2, s2, d2, after_vel);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamWaitEvent(after_vel, e->mir_ev3, 0));
        HIPCHK(e, hipEventRecord(e->mir_ev2, after_vel));  // no mirror kernel reads the state
        HIPCHK(e, hipStreamWaitEvent(ms, e->mir_ev2, 0));
        for (int j : {2, 3})
            HIPCHK(e, hipMemcpyAsync(e->mir + j * c, st + j * c, sizeof(double) * n,
                                     hipMemcpyDeviceToHost, ms));
    } else {
        HIPCHK(e, hipEventRecord(e->mir_ev2, after_vel));
        HIPCHK(e, hipStreamWaitEvent(ms, e->mir_ev2, 0));
    }
    HIPCHK(e, hipEventRecord(e->mir_ev, ms));
    e->mir_launched = true;
    return BH_OK;
}

int mirror_launch(bh_engine *e, const BodyState &src, hipStream_t after_pos, hipStream_t after_vel) {
    TRY(mirror_pos(e, src, after_pos));
    return mirror_vel(e, src, after_vel);
}

// The second evaluation of a pipelined step: build, second traversal with the fused kick, and
// next step's first build; e->prebuilt tells the next evaluation its tree is there.
// Order on the device:
//   engine's stream:  build ... k_emit_com | k_span_children, k_com_span (_top) | traversal | join
//   overlap stream:                        | [removal count] merge rule, next build's sort |
//                                            ... its k_fixup_cells onwards (after the span
//                                            passes)
// The host enqueues the chain after the traversal (lastTree's buffer swap lies between the span
// passes' launch and the overlapped build's); the events alone decide where it runs.
// last: the call's last step -- this step's tree is lastTree (BHA:435): its walk structures are
// copied aside before the overlapped build reuses them, and the state before that build's jitter
// (the previous slot order) becomes the caller-visible `view`.
int evaluate_pipelined(bh_engine *e, bool last) {
    const int64_t n = e->n;
    hipStream_t s = e->stream;
    // the merge rule's mailbox header is cleared by the build's k_emit_com, or by k_trav_inputs
    // below (after the previous merge rule, which the engine's stream waited for, and before the
    // overlapped one, which forks behind whichever of the two ran): a fill of its own sat on the
    // engine's hardware queue between the build and the traversal
    const bool merging = e->p.merge_min_dist > 0.0 && e->n > 1 && e->heavy_possible;
    if (merging) TRY(merge_bufs(e));
    TRY(mark(e, -1));
    if (e->lr_ready) {  // the re-sorted lane map (prebuilt order), carried on by this build
        HIPCHK(e, hipStreamWaitEvent(s, e->lr_ev, 0));
        std::swap(e->lanes, e->lanes_next);
        e->lr_ready = false;
        e->lanes_age = 0;
    }
    BuildRequest b2{};        // the second build: in place on the engine's stream
    b2.keep_v = true;         // velocities: permuted by the kick below
    b2.heavy_list = merging;  // for the merge rule that follows
    b2.lane_hold = true;      // a due lane re-sort waits for the next first traversal's side
    // the second traversal's input copies (masses, flags, lane map, node count) written by this
    // build's k_emit_com instead of a k_trav_inputs launch between the build and the traversal
    b2.tc_want = true;
    b2.tc_box = merging ? reinterpret_cast<uint32_t *>(e->box) : nullptr;
    // With the mirror on, a call's last step runs the merge rule and the mirror's caller-order
    // gather of positions and masses before the traversal (~0.15 ms in line): the mirror's 40 MB
    // cross PCIe from then on instead of from when the overlapped merge rule and gather find wave
    // slots beside the traversal, ~0.45 ms later (round 4 drop-in trace)
    const bool early = last && e->mirror_on;
    // The overlapped chain forks at the end of the build's k_emit_com: the sorted positions, the
    // heavy list and the traversal's own copies of masses and flags are final there, the mailbox
    // header is cleared, and only the spanning passes (one workgroup on one CU for most of their
    // ~50 us) stand between the build and the traversal.  The merge rule and the next build's
    // sort run in that window on an otherwise idle GPU instead of waiting for wave slots beside
    // the traversal.  Not when the build leaves the copies to k_trav_inputs (a re-sorted lane
    // map): that kernel reads the masses and flags the rule writes, so the chain starts after it.
    b2.fork_want = early ? nullptr : e->pipe_ev[2];
    TRY(build_into(e, s, b2));
    TRY(mark(e, 0));
    // with profiling on, the overlapped chain waits for the timing event just recorded after the
    // build (when nothing else follows the build on this stream): each event recorded on the
    // stream holds the next kernel back by a few microseconds
    const hipEvent_t built_mark =
        e->profiling && e->ev_used > 0 && b2.tc_done ? e->ev[e->ev_used - 1] : nullptr;
    const bool lanes = e->lanes_valid;
    if (!b2.tc_done) {  // (the build made them otherwise)
        copy_trav_inputs(n, e->st.m, e->m_trav, e->st.cidx, e->cidx_trav,
                         lanes ? e->lanes : nullptr, e->lanes_trav, e->base + n, e->T_trav, s,
                         merging ? e->box : nullptr);
        HIPCHK(e, hipGetLastError());
    }
    if (early) {
        copy_u32(e->scalars + 8, e->scalars + 2, s);  // the removals before the last merge rule
        HIPCHK(e, hipGetLastError());
        TRY(merge(e, s, merging));  // BHA:438 (the traversal reads its own copies of m, cidx)
        TRY(mirror_pos(e, e->st, s, true));
        if (e->mid_armed && e->mir_idx && n > 0) {  // bh_step_positions: the hand-off
            HIPCHK(e, hipEventRecord(e->mid_ev, e->mir_stream));
            {
                std::lock_guard<std::mutex> lk(e->mid_mu);
                e->mid_buf = e->mir;
                e->mid_stride = e->mir_cap;
                e->mid_ready = true;
            }
            e->mid_cv.notify_all();
        }
    }
    BuildRequest b1{};  // step s+1's first tree (BHA:359), beside the traversal
    b1.overlap = true;
    b1.carry = last;
    b1.lane_defer = !last;  // (a call ends with a compaction: its last build re-sorts in place)
    if (b2.forked) {
        // the chain starts behind k_emit_com; from its build's first kernel that writes the span
        // lists on it waits for this build's spanning passes (the event after the build)
        HIPCHK(e, hipStreamWaitEvent(e->pipe_stream, e->pipe_ev[2], 0));
        if (built_mark) {
            b1.chain_late = built_mark;
        } else {
            HIPCHK(e, hipEventRecord(e->pipe_ev[0], s));
            b1.chain_late = e->pipe_ev[0];
        }
    } else if (built_mark && !early) {
        HIPCHK(e, hipStreamWaitEvent(e->pipe_stream, built_mark, 0));
    } else {
        HIPCHK(e, hipEventRecord(e->pipe_ev[0], s));
        HIPCHK(e, hipStreamWaitEvent(e->pipe_stream, e->pipe_ev[0], 0));
    }
    const ForceParams fp = force_params(e);  // BHA:378
    KickArgs ka{KICK_ONLY, e->st.vx, e->st.vy, e->p.dt * 0.5, e->p.dt};
    if (n > 0) {  // (the build swapped: the previous order's velocities are in alt)
        ka.svx = e->alt.vx;
        ka.svy = e->alt.vy;
        ka.perm = e->perm;
    }
    WaveOrder wo;
    TRY(wave_order_for(e, 0, n, s, wo));
    // (with the step log on: the same walk with every body's potential, by slot)
    traverse(e->nodes, e->node_cap, e->T_trav, e->st.x, e->st.y, e->m_trav, e->cidx_trav, 0, n,
             e->geo, fp, e->a2, nullptr, s, &ka, lanes ? e->lanes_trav : nullptr, &wo,
             e->slog_cap > 0 ? e->slog_phi : nullptr);
    HIPCHK(e, hipGetLastError());
    TRY(mark(e, 1));
    TRY(wave_order_next(e, 0, n, s));
    // the step's record from the traversal's own copies of masses and flags (the merge rule --
    // before the traversal on the mirror's early path, beside it otherwise -- writes st.m and
    // st.cidx) and the positions and kicked velocities in st, on this stream before the swap
    TRY(step_log_step(e, e->cidx_trav, e->m_trav));
    // the tracers on the tree and node count the traversal just read (the overlapped chain
    // writes the other node array, the masses and the flags: none of them read here)
    TRY(tracer_walk(e, e->nodes, e->node_cap, e->T_trav, KICK_ONLY));
    if (last) {
        hipStream_t ps = e->pipe_stream;
        // lastTree's walk (bh_get_quads): this build's sorted keys, prefix lengths and node
        // offsets stay where they are, the overlapped build below writes the other set (a copy
        // aside ran as a blit beside the traversal: ~0.5 ms, with the merge rule queued behind it)
        std::swap(e->keys_s, e->lt_keys);
        std::swap(e->cpl, e->lt_cpl);
        std::swap(e->base, e->lt_base);
        if (!early) {  // the call's removal count before its last merge rule (BHA:526)
            copy_u32(e->scalars + 8, e->scalars + 2, ps);
            HIPCHK(e, hipGetLastError());
        }
    }
    if (!early) TRY(merge(e, e->pipe_stream, merging));  // BHA:438
    if (early) TRY(mirror_vel(e, e->st, s));  // the velocities once the kick is done
    TRY(build_into(e, e->pipe_stream, b1));
    HIPCHK(e, hipEventRecord(e->pipe_ev[1], e->pipe_stream));
    HIPCHK(e, hipStreamWaitEvent(s, e->pipe_ev[1], 0));
    if (!last) {
        e->vel_perm = e->perm2;  // the next step's first kick reads them through the permutation
    } else {
        permute_velocities(n, e->perm2, e->st.vx, e->st.vy, e->alt.vx, e->alt.vy, s);
        HIPCHK(e, hipGetLastError());
    }
    TRY(mark(e, 0));  // the wait for the overlapped build and the velocity permutation
    std::swap(e->st, e->alt);
    std::swap(e->nodes, e->nodes_alt);
    std::swap(e->node_cap, e->nodes_alt_cap);
    e->prebuilt = true;
    e->carried_flags = last;
    if (last) {  // the previous order's state (kicked, merged, not yet jittered) is what the caller sees
        std::swap(e->view, e->alt);
        e->view_pending = true;
        e->lt_aside = true;
    }
    return BH_OK;
}

// The positions the call's last build starts from (its jitter moves some of them): kept for the
// lazy lastTree of bh_get_quads (16 B per body, device copies).
int snapshot_positions(bh_engine *e) {
    const int64_t n = e->n;
    TRY(materialize_positions(e));
    if (e->lt_cap < e->cap) {
        TRY(dev_alloc(e, e->lt_x, (size_t)e->cap));
        TRY(dev_alloc(e, e->lt_y, (size_t)e->cap));
        e->lt_cap = e->cap;
    }
    if (n > 0) {
        HIPCHK(e, hipMemcpyAsync(e->lt_x, e->st.x, sizeof(double) * n, hipMemcpyDeviceToDevice,
                                 e->stream));
        HIPCHK(e, hipMemcpyAsync(e->lt_y, e->st.y, sizeof(double) * n, hipMemcpyDeviceToDevice,
                                 e->stream));
    }
    return BH_OK;
}

// The lane map's due Hilbert re-order (build_into), from the prebuilt tree's sorted keys, on the
// overlap stream beside the first traversal -- which walks the map carried through that build --
// into lanes_next, swapped in before the second build carries it on (evaluate_pipelined).  The
// traversal writes none of these buffers (its fused epilogue writes keys / keys32, not keys_s).
// Made in the overlapped build, the re-sort ran after the chain and outlasted the second
// traversal by ~0.12 ms once every 8 steps (round 4 timeline).
int lane_refresh_beside(bh_engine *e) {
    e->lr_pending = false;
    const int64_t n = e->n;
    if (n <= 0 || !e->lanes_valid) return BH_OK;
    if (e->lr_cap < e->cap) {
        for (uint32_t **q : {&e->lanes_next, &e->lr_hkey, &e->lr_hkey_s, &e->lr_slot}) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        if (e->lr_scratch) (void)hipFree(e->lr_scratch);
        e->lr_scratch = nullptr;
        e->lr_cap = 0;
        for (uint32_t **q : {&e->lanes_next, &e->lr_hkey}) TRY(dev_alloc(e, *q, (size_t)e->cap));
        if (e->lane_sort)  // (the radix sort's second key buffer and its slot values)
            for (uint32_t **q : {&e->lr_hkey_s, &e->lr_slot}) TRY(dev_alloc(e, *q, (size_t)e->cap));
        e->lr_scratch_bytes = lane_sort_bytes(e->cap);
        HIPCHK(e, hipMalloc(&e->lr_scratch, e->lr_scratch_bytes));
        e->lr_cap = e->cap;
    }
    if (!e->lr_ev) HIPCHK(e, hipEventCreateWithFlags(&e->lr_ev, kPipeEvFlags));
    HIPCHK(e, lane_order_into(e->keys_s, n, e->geo.J, e->lr_hkey, e->lr_hkey_s, e->lr_slot,
                              e->lr_scratch, e->lr_scratch_bytes, e->lanes_next, e->pipe_stream,
                              e->lane_sort));
    HIPCHK(e, hipEventRecord(e->lr_ev, e->pipe_stream));
    e->lr_ready = true;
    return BH_OK;
}

// ---- one PhysicsEngine.step() (BHA:405-439) ------------------------------------------
// last: the final step of a bh_step call -- its second build is the full tree (lastTree,
// BHA:435, for getTreeForDebug) also on a multi-rank engine that shards its builds.
int step_once(bh_engine *e, bool last) {
    const int64_t n = e->n;
    const double dtHalf = e->p.dt * 0.5;  // BHA:412
    if (pipelined(e)) {
        TRY(pipe_alloc(e, last));
        if (e->lr_pending && e->prebuilt) TRY(lane_refresh_beside(e));
        e->lr_pending = false;
        bool fused = false;
        e->fuse_keys = true;  // and the second build's keys and bucket counts
        TRY(evaluate(e, nullptr, KICK_DRIFT, &fused, true));  // a(t), kick + drift fused
        if (!fused) {
            e->err = "pipelined step: the first evaluation did not fuse its kick";
            return BH_E_STATE;
        }
        // the tracers on the tree that evaluation walked; the in-place second build follows
        TRY(tracer_walk(e, e->nodes, e->node_cap, e->base + n, KICK_DRIFT));
        TRY(evaluate_pipelined(e, last));  // a(t+dt), the kick, the merge rule and the next tree
        e->tree_valid = true;
        return BH_OK;
    }
    if (n > 0) {
        bool fused = false;  // one GPU: the kicks ride in the traversal's epilogue
        // (multi-rank LET evaluations integrate their own bodies too: fused)
        TRY(evaluate(e, nullptr, KICK_DRIFT, &fused, true));  // a(t)
        if (!fused) {
            TRY(mark(e, -1));
            kick_drift(n, e->a2, e->st.x, e->st.y, e->st.vx, e->st.vy, dtHalf, e->p.dt,
                       e->stream, e->a2_lanes, e->a2_layout, e->boxes_valid ? e->L.vmax : nullptr);
            HIPCHK(e, hipGetLastError());
            if (e->boxes_valid) {  // every rank drifted every body: its own bound is everyone's
                let_disp_add(e->disp, e->L.vmax, e->L.nvmax, e->p.dt, e->stream);
                HIPCHK(e, hipGetLastError());
            }
            TRY(mark(e, 2));
        }
        TRY(tracer_walk(e, e->nodes, e->node_cap, e->base + n, KICK_DRIFT));
        // the call's last build: a full tree for getTreeForDebug (lastTree, BHA:435) -- or, on a
        // multi-rank engine, a LET build like the others, its input positions kept for a lazy
        // full build in bh_get_quads
        const bool lazy = last && (e->comm || e->group || e->solo);
        if (lazy) TRY(snapshot_positions(e));
        bool let2 = false;
        TRY(evaluate(e, nullptr, KICK_ONLY, &fused, !last || lazy, &let2));  // a(t+dt)
        if (!fused) {
            TRY(mark(e, -1));
            kick(n, e->a2, e->st.vx, e->st.vy, dtHalf, e->stream, e->a2_lanes, e->a2_layout);
            HIPCHK(e, hipGetLastError());
            TRY(mark(e, 2));
        }
        TRY(tracer_walk(e, e->nodes, e->node_cap, e->base + n, KICK_ONLY));
        if (e->slog_cap > 0) {  // (one GPU, not pipelined: theta = 0, the all-pairs evaluation)
            if (!theta2_is_zero(e)) {
                e->err = "step log: a tree walk outside the pipelined step";
                return BH_E_STATE;
            }
            // the potential over the evaluation's leaf list (bit-identical to the walk at theta 0)
            direct_potential(e->leaves, e->leaf_count, e->st.x, e->st.y, e->st.cidx, n, e->p.G,
                             e->p.soft2, e->slog_phi, e->stream);
            HIPCHK(e, hipGetLastError());
            TRY(step_log_step(e, e->st.cidx, e->st.m));
        }
        e->tree_valid = !let2;  // lastTree = root (BHA:435)
        e->lazy_tree = lazy && let2;
    } else {  // no bodies, no tree: every sum is +0.0 and the tracers drift on straight lines
        TRY(tracer_walk(e, nullptr, 0, nullptr, KICK_DRIFT));
        TRY(tracer_walk(e, nullptr, 0, nullptr, KICK_ONLY));
        TRY(step_log_step(e, nullptr, nullptr));  // an all-zero record: step and t advance
    }
    if (last)  // the call's removal count before its last merge rule (finish_merges, BHA:526)
        HIPCHK(e, hipMemcpyAsync(e->scalars + 8, e->scalars + 2, sizeof(uint32_t),
                                 hipMemcpyDeviceToDevice, e->stream));
    return merge(e);  // BHA:438
}

// ---- getTreeForDebug().visitQuads (BHA:265-274) from the Morton structure ------------
struct QuadWalker {
    const Geometry &g;
    const std::vector<uint64_t> &keys;
    const std::vector<int8_t> &cpl;
    const std::vector<uint32_t> &base;
    const Node *nodes;  // device
    double *cx, *cy, *h;
    int64_t cap, k = 0;
    int rc = BH_OK;

    void emit(double qx, double qy, double qh) {
        if (k < cap) {
            cx[k] = qx;
            cy[k] = qy;
            h[k] = qh;
        }
        ++k;
    }
    static void child(double qx, double qy, double qh, int which, double &ox, double &oy,
                      double &oh) {  // BHA:73-81
        double hh = qh / 2.0;
        ox = (which & 1) ? qx + hh : qx - hh;
        oy = (which & 2) ? qy + hh : qy - hh;
        oh = hh;
    }
    void leaf_children(double qx, double qy, double qh) {
        for (int q = 0; q < 4; ++q) {
            double ox, oy, oh;
            child(qx, qy, qh, q, ox, oy, oh);
            emit(ox, oy, oh);
        }
    }
    void rec(int L, int64_t lo, int64_t hi, double qx, double qy, double qh) {
        emit(qx, qy, qh);
        if (hi - lo < 2) return;  // empty or single-body leaf
        if (L == g.J) {           // jitter cell: children from the replay
            int cp = lo > 0 ? (int)cpl[lo - 1] : -1;
            uint32_t ni = base[lo] + (uint32_t)(L - cp - 1);
            Node nd;
            if (hipMemcpy(&nd, nodes + ni, sizeof(Node), hipMemcpyDeviceToHost) != hipSuccess) {
                rc = BH_E_DEVICE;
                return;
            }
            uint32_t jmask = (nd.meta >> NODE_JMASK_SHIFT) & 0xFu;
            for (int q = 0; q < 4; ++q) {
                double ox, oy, oh;
                child(qx, qy, qh, q, ox, oy, oh);
                emit(ox, oy, oh);
                if (jmask & (1u << q)) leaf_children(ox, oy, oh);
            }
            return;
        }
        const int shift = 2 * (g.J - 1 - L);
        int64_t s = lo;
        for (int q = 0; q < 4; ++q) {
            int64_t e2 = s;
            while (e2 < hi && (int)((keys[e2] >> shift) & 3u) == q) ++e2;
            double ox, oy, oh;
            child(qx, qy, qh, q, ox, oy, oh);
            rec(L + 1, s, e2, ox, oy, oh);
            s = e2;
        }
    }
};

void set_defaults(bh_params *p) {
    p->G = 80.0;                 // CFG:11
    p->dt = 0.005;               // CFG:14
    p->theta = 0.30;             // CFG:23
    p->soft2 = 1.0 * 1.0;        // CFG:17,20
    p->width_px = 2400;          // CFG:5
    p->height_px = 800;          // CFG:8
    p->merge_max_mass = 4000.0;  // BHA:315
    p->merge_min_dist = 8.0;     // BHA:321 = Config.MIN_R (CFG:35)
}

int engine_init(bh_engine *e, const bh_params *p, int device) {
    if (!p) {
        e->err = "params is NULL";
        return BH_E_INVALID;
    }
    e->p = *p;
    TRY(make_geometry(e->p, e->geo, e->err));
    e->device = device;
    if (const char *v = std::getenv("BH_LET")) {
        e->let_on = std::strcmp(v, "0") != 0;
        e->let_forced = std::strcmp(v, "1") == 0;
    }
    if (const char *v = std::getenv("BH_LANE_ORDER_SORT")) e->lane_sort = std::strcmp(v, "1") == 0;
    HIPCHK(e, hipSetDevice(device));
    HIPCHK(e, hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    TRY(dev_alloc(e, e->scalars, 16));
    HIPCHK(e, hipMemsetAsync(e->scalars, 0, 16 * sizeof(uint32_t), e->stream));
    TRY(ensure_capacity(e, 1));
    return BH_OK;
}

void free_state(BodyState &s) {
    void *p[] = {s.x, s.y, s.vx, s.vy, s.m, s.cidx};
    for (void *q : p)
        if (q) (void)hipFree(q);
}

}  // namespace

// Round sizes of a rank's lane range (BH_ROUND_FRACS="a,b,c,d": relative weights; default
// below): whole wavefronts, the same on every rank (bh_shard_range, bh_gather_slot).
static const double *round_cum() {
    struct Cum {
        double c[BH_SHARD_ROUNDS + 1];
        Cum() {
            double w[BH_SHARD_ROUNDS] = {BH_ROUND_WEIGHTS};
            if (const char *v = std::getenv("BH_ROUND_FRACS")) {
                double t[BH_SHARD_ROUNDS];
                int k = 0;
                const char *p = v;
                while (k < BH_SHARD_ROUNDS && *p) {
                    char *end = nullptr;
                    t[k] = std::strtod(p, &end);
                    if (end == p || !(t[k] > 0.0)) break;
                    ++k;
                    p = *end == ',' ? end + 1 : end;
                }
                if (k == BH_SHARD_ROUNDS)
                    for (int j = 0; j < k; ++j) w[j] = t[j];
            }
            double tot = 0.0;
            for (double x : w) tot += x;
            c[0] = 0.0;
            for (int j = 0; j < BH_SHARD_ROUNDS; ++j) c[j + 1] = c[j] + w[j] / tot;
        }
    };
    static const Cum cum;  // thread-safe initialisation (the in-process ranks are threads)
    return cum.c;
}

GatherLayout bh::shard_layout(int64_t n, int world) {
    GatherLayout L{};
    const int64_t sub = shard_sub(n, world, BH_SHARD_ROUNDS);
    L.span = sub * BH_SHARD_ROUNDS;
    L.world = world;
    const double *cum = round_cum();
    L.off[0] = 0;
    for (int k = 1; k < BH_SHARD_ROUNDS; ++k)
        L.off[k] = std::max<int64_t>(L.off[k - 1],
                                     std::min<int64_t>(L.span, (int64_t)(cum[k] * (double)L.span) / 64 * 64));
    L.off[BH_SHARD_ROUNDS] = L.span;
    return L;
}

void bh::set_error(bh_engine *e, const std::string &msg) {
    if (e) e->err = msg;
}

// The per-process settings that decide which collectives a step issues and how large each piece
// is -- BH_LET (LET builds: the cell-table all-gather) and BH_ROUND_FRACS (the round sizes of
// bh_shard_range / bh_gather_slot) -- must be equal on every rank, or the collectives stop
// matching and the run hangs.  Min- and max-reduced over the ranks at creation: every rank sees
// the same comparison, so all of them fail together on a mismatch.
static int agree_settings(bh_engine *e) {
    constexpr int K = 2 + BH_SHARD_ROUNDS + 1;
    double v[K];
    v[0] = e->let_on ? 1.0 : 0.0;
    v[1] = e->let_forced ? 1.0 : 0.0;
    const double *cum = round_cum();
    for (int j = 0; j <= BH_SHARD_ROUNDS; ++j) v[2 + j] = cum[j];
    // device scratch from the engine's own buffers (allocated by ensure_capacity: no allocation
    // that could fail on one rank only), and every rank takes part in both all-reduces whatever
    // happened locally, so a local failure cannot leave the peers waiting in a collective
    double *d = static_cast<double *>(e->scratch);
    double lo[K], hi[K];
    TRY(coll_log(e, COLL_SETTINGS, (int64_t)sizeof(double) * 2 * K, CS_MAIN));
    ncclResult_t nr = ncclSuccess;
    if (!d || e->scratch_bytes < sizeof(double) * 3 * K) {
        e->err = "agree_settings: no device scratch";
        return BH_E_STATE;  // (every rank: the buffers are sized alike)
    }
    hipError_t hr = hipMemcpyAsync(d, v, sizeof(v), hipMemcpyHostToDevice, e->stream);
    if (hr != hipSuccess)  // NaN bit patterns (if the device still takes a fill): no match
        (void)hipMemsetAsync(d, 0xFF, sizeof(v), e->stream);
    ncclResult_t n1 = ncclAllReduce(d, d + K, K, ncclFloat64, ncclMin, e->comm, e->stream);
    ncclResult_t n2 = ncclAllReduce(d, d + 2 * K, K, ncclFloat64, ncclMax, e->comm, e->stream);
    nr = n1 != ncclSuccess ? n1 : n2;
    hipError_t h2 = hipMemcpyAsync(lo, d + K, sizeof(lo), hipMemcpyDeviceToHost, e->stream);
    if (h2 == hipSuccess) h2 = hipMemcpyAsync(hi, d + 2 * K, sizeof(hi), hipMemcpyDeviceToHost, e->stream);
    if (h2 == hipSuccess && wait_stream(e, e->stream) != BH_OK) return BH_E_COMM;  // (bounded)
    if (hr == hipSuccess) hr = h2;
    if (nr != ncclSuccess) {
        e->err = std::string("agree_settings: ") + ncclGetErrorString(nr);
        return BH_E_COMM;
    }
    if (hr != hipSuccess) {
        e->err = std::string("agree_settings: ") + hipGetErrorString(hr);
        return BH_E_DEVICE;
    }
    for (int j = 0; j < K; ++j)
        if (lo[j] != hi[j]) {
            e->err = "BH_LET / BH_ROUND_FRACS differ between ranks: every rank must run with the "
                     "same settings";
            return BH_E_INVALID;
        }
    return BH_OK;
}

// ---- the multi-device handle's pieces (multi.hpp) -----------------------------------------
#ifndef BH_MULTI_MIN_BODIES
// body lists below this run on one GPU behind a multi-device handle.  A LET evaluation costs ~40
// launches of >= 4.5 us per build (two per step) plus 8 round launches and the exchanges
// whatever the size, ~0.6 ms per step; one GPU steps 1e5 bodies in 0.55 ms and 1e6 in 1.8 ms,
// so the split pays from a few 1e5 bodies on (an estimate: no multi-GPU box was available).
#define BH_MULTI_MIN_BODIES 400000
#endif
int bh::facade_create(const bh_params *p, bh::Multi *mu, bh_engine **out) {
    bh_engine *f = new bh_engine();
    f->p = *p;
    if (make_geometry(f->p, f->geo, f->err) != BH_OK) {
        delete f;
        return BH_E_INVALID;
    }
    f->multi = mu;
    f->world = multi_world(mu);
    f->multi_min = 0;
    if (const char *v = std::getenv("BH_MULTI_MIN_BODIES")) f->multi_min = std::atoll(v);
    else f->multi_min = BH_MULTI_MIN_BODIES;
    *out = f;
    return BH_OK;
}

int bh::member_agree(bh_engine *e) {
    if (!e->comm) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));  // (a pool thread: RCCL calls on the member's device)
    return agree_settings(e);
}

void bh::member_set_abort(bh_engine *e, std::atomic<bool> *flag) { e->abort_flag = flag; }

void bh::member_drop_comm(bh_engine *e) {
    if (e->comm) {
        (void)hipSetDevice(e->device);
        (void)ncclCommAbort(e->comm);
        e->comm = nullptr;
        e->comm_lost = true;
    }
}

void bh::member_set_comm(bh_engine *e, void *comm) {
    e->comm = static_cast<ncclComm_t>(comm);
    e->comm_lost = false;
}

// (comm: an RCCL communicator made in this process; on failure it stays the caller's)
int bh::member_create(const bh_params *p, int device, int rank, int world, void *comm,
                      bh_local_group *group, bh_engine **out) {
    if (group) return bh_create_local(p, device, rank, group, out);
    if (!out || !comm || world < 1 || rank < 0 || rank >= world) return BH_E_INVALID;
    *out = nullptr;
    bh_engine *e = new bh_engine();
    e->rank = rank;
    e->world = world;
    int rc = engine_init(e, p, device);
    if (rc == BH_OK) {
        e->comm = static_cast<ncclComm_t>(comm);
        hipError_t hr = comm_stream_create(&e->comm_stream);
        for (int k = 0; k < BH_SHARD_ROUNDS && hr == hipSuccess; ++k)
            hr = hipEventCreateWithFlags(&e->round_ev[k], hipEventDisableTiming);
        if (hr == hipSuccess) hr = hipEventCreateWithFlags(&e->gathered_ev, hipEventDisableTiming);
        if (hr != hipSuccess) {
            e->err = std::string("comm stream/events: ") + hipGetErrorString(hr);
            rc = BH_E_DEVICE;
        }
    }
    if (rc == BH_OK) {  // the accelerations buffer in rounds x world pieces
        const int64_t cap = e->cap;
        e->cap = 0;
        rc = ensure_capacity(e, cap);
    }
    if (rc != BH_OK) {
        std::fprintf(stderr, "bh_create_multi (rank %d): %s\n", rank, e->err.c_str());
        e->comm = nullptr;
        bh_destroy(e);
        return rc;
    }
    *out = e;
    return BH_OK;
}

// getTreeForDebug (BHA:329-332): lastTree if the last step kept it, else a fresh tree -- built
// here, its jitter applied to the state as the reference's buildTree applies it.
int bh::quads_prepare(bh_engine *e) {
    HIPCHK(e, hipSetDevice(e->device));
    const int64_t n = e->n;
    TRY(materialize_positions(e));
    if (!e->tree_valid && (e->comm || e->group || e->solo)) {
        // multi-rank: the tree is built into the workspace from the positions of the call's last
        // build (the lazy lastTree) or the current ones (getTreeForDebug's fresh tree), and the
        // state stays as it is -- a rank's slot order and lane map must not change on its own
        HIPCHK(e, hipMemsetAsync(e->scalars + 1, 0, sizeof(uint32_t), e->stream));
        if (n > 0) {
            TreeBuffers tb = tree_buffers(e);
            if (e->lazy_tree) {
                tb.src.x = e->lt_x;
                tb.src.y = e->lt_y;
            }
            tb.src.vx = tb.src.vy = nullptr;  // positions, masses and flags are all it reads
            tb.spl_nb = 0;                    // the caller's splitters describe another order
            tb.lanes_remap = nullptr;
            HIPCHK(e, tree_build(tb, n, e->geo, e->stream));
            if (!e->lazy_tree) {
                // getTreeForDebug's fresh buildTree moves the bodies it jitters (BHA:146-151,
                // 329-331): the moved positions go back into the replica in its own slot order
                // (every rank makes the same calls, so the replicas stay equal)
                unpermute_positions(n, e->perm, tb.dst.x, tb.dst.y, e->st.x, e->st.y, e->stream);
                HIPCHK(e, hipGetLastError());
                e->mir_fresh = false;
                ++e->builds_since_box;  // (its jitter, for the LET selection's bound)
            }
            e->spl_nb = 0;  // k_prep wrote splitters of this order
            e->keys_ready = false;
            TRY(check_tree_flags(e));
        } else {
            HIPCHK(e, hipMemsetAsync(e->base, 0, sizeof(uint32_t), e->stream));
        }
        e->tree_valid = true;  // until the next step (a second call walks the same tree)
    } else if (!e->tree_valid && e->view_pending) {
        // getTreeForDebug's fresh tree (BHA:329-332) is the one the pipelined call already built
        // from the caller's bodies after its merge rule: its jitter becomes part of the state, and
        // the next step builds its own first tree from these positions (BHA:407)
        e->view_pending = false;
        e->prebuilt = false;
        e->mir_fresh = false;
        e->tree_valid = true;
        HIPCHK(e, hipMemsetAsync(e->scalars + 1, 0, sizeof(uint32_t), e->stream));
        TRY(take_carried_flags(e));
        if (n > 0) TRY(check_tree_flags(e));
    } else if (!e->tree_valid) {  // getTreeForDebug builds a fresh tree (BHA:329-332)
        HIPCHK(e, hipMemsetAsync(e->scalars + 1, 0, sizeof(uint32_t), e->stream));
        TRY(build(e));
        if (n > 0) TRY(check_tree_flags(e));
    }
    return BH_OK;
}

// A multi-device handle's calls: on the engine that holds the bodies -- every member, or the
// single-GPU engine of a small body list -- and, for the settings (params, profiling, mirror),
// on both, so that either is current when a reset switches between them.
namespace {
int multi_fan(bh_engine *e, const std::function<int(bh_engine *, int)> &fn, bool both) {
    int rc = BH_OK;
    if (e->use_one) {
        rc = fn(e->one, 0);
        if (rc != BH_OK) e->err = bh_last_error(e->one);
    }
    if (!e->use_one || both) {
        const int r2 = multi_all(e->multi, e, fn);
        if (rc == BH_OK) rc = r2;
    }
    if (both && !e->use_one && e->one && rc == BH_OK) {
        rc = fn(e->one, 0);
        if (rc != BH_OK) e->err = bh_last_error(e->one);
    }
    return rc;
}
bh_engine *multi_active0(const bh_engine *e) { return e->use_one ? e->one : multi_member(e->multi, 0); }
}  // namespace
#define MULTI_FAN(e, both, call)                                                        \
    do {                                                                                \
        if ((e)->multi)                                                                 \
            return multi_fan((e), [&](bh_engine *m_, int r_) {                          \
                (void)r_;                                                               \
                return call;                                                            \
            }, both);                                                                   \
    } while (0)
#define MULTI_ALL(e, call) MULTI_FAN(e, false, call)
#define MULTI_BOTH(e, call) MULTI_FAN(e, true, call)
// the calls that only read the state: the active engine's member 0 (every replica is complete at
// the API boundary)
#define MULTI_M0(e) ((e)->multi ? multi_active0(e) : (e))

// A call begun by bh_step_begin owns the engine until bh_step_end: the other calls that use
// the engine are refused (BH_E_STATE, without touching the error text the call may be writing)
// from any thread but the call's own.
#define ASYNC_GUARD(e)                                                                         \
    do {                                                                                       \
        if ((e)->async_running && std::this_thread::get_id() != (e)->step_thr.get_id())      \
            return BH_E_STATE;                                                                 \
    } while (0)

// A rank of a decomposition whose last call failed -- here or on a peer (the group / handle was
// aborted) -- refuses the calls that use the replica or issue collectives until bh_reset_bodies:
// every rank refuses alike, so none waits in a collective the others never issue.
namespace {
int comm_refused(bh_engine *e) {
    if (!multi_rank(e) || (!e->comm_failed && !peers_aborted(e))) return BH_OK;
    e->err = "a previous call of this multi-rank engine failed (" +
             (e->comm_failed ? e->fail_msg : std::string("on a peer rank")) +
             "); bh_reset_bodies before the next call";
    return BH_E_COMM;
}
}  // namespace
#define COMM_GUARD(e) TRY(comm_refused(e))

// A tree query, written as query(engine, run), on the handle the caller holds.  Every member of a
// multi-device handle runs it -- each builds, so that the build jitters every replica alike --
// and member 0 alone evaluates and answers (run = true); any other engine is its own member 0.
// Each engine passes its guards first, and a failure marks a multi-rank engine failed.
namespace {
int query_call(bh_engine *e, const std::function<int(bh_engine *, bool)> &query) {
    auto guarded = [&](bh_engine *m, int r) -> int {
        ASYNC_GUARD(m);
        COMM_GUARD(m);
        return fail_multi_rank(m, query(m, r == 0));
    };
    return e->multi ? multi_fan(e, guarded, false) : guarded(e, 0);
}

// A list argument of `fn`: the count `what` = n must be in [0, 2^28] and, unless it is 0, the
// arrays that `arrays` names must be there (have).
int check_list(bh_engine *e, const char *fn, const char *what, int64_t n, bool have,
               const char *arrays) {
    if (n < 0 || n > ((int64_t)1 << 28)) {
        e->err = std::string(fn) + ": " + what + " must be in [0, 2^28]";
        return BH_E_INVALID;
    }
    if (n > 0 && !have) {
        e->err = std::string(fn) + ": " + arrays + " is NULL";
        return BH_E_INVALID;
    }
    return BH_OK;
}
}  // namespace

// =========================================================================================
extern "C" {

static int last_removed(const bh_engine *e, int64_t *idx, int64_t cap, int64_t *n_out);

void bh_default_params(bh_params *p) {
    if (p) set_defaults(p);
}

int bh_create(const bh_params *p, int device, bh_engine **out) {
    if (!out) return BH_E_INVALID;
    *out = nullptr;
    bh_engine *e = new bh_engine();
    int rc = engine_init(e, p, device);
    // the overlap stream right after the engine's own (HIP hands a process's few hardware queues
    // out in stream creation order); the mirror's is made by bh_set_mirror, which a caller that
    // reads the mirror calls right after bh_create (the shims do)
    if (rc == BH_OK) rc = pipe_streams(e);
    if (rc != BH_OK) {
        std::fprintf(stderr, "bh_create: %s\n", e->err.c_str());
        bh_destroy(e);
        return rc;
    }
    *out = e;
    return BH_OK;
}

int bh_comm_unique_id(void *out128) {
    if (!out128) return BH_E_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return BH_E_COMM;
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id must be 128 bytes");
    std::memcpy(out128, &id, sizeof(id));
    return BH_OK;
}

int bh_create_dist(const bh_params *p, int device, int rank, int world, const void *unique_id,
                   bh_engine **out) {
    if (!out || world < 1 || rank < 0 || rank >= world || (world > 1 && !unique_id))
        return BH_E_INVALID;
    *out = nullptr;
    bh_engine *e = new bh_engine();
    e->rank = rank;
    e->world = world;
    int rc = engine_init(e, p, device);
    if (rc == BH_OK && unique_id) {  // world == 1 with an id: the RCCL path on one rank
        ncclUniqueId id;
        std::memcpy(&id, unique_id, sizeof(id));
        ncclResult_t nr = ncclCommInitRank(&e->comm, world, id, rank);
        if (nr != ncclSuccess) {
            e->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(nr);
            rc = BH_E_COMM;
        }
        hipError_t hr = comm_stream_create(&e->comm_stream);
        for (int k = 0; k < BH_SHARD_ROUNDS && hr == hipSuccess; ++k)
            hr = hipEventCreateWithFlags(&e->round_ev[k], hipEventDisableTiming);
        if (hr == hipSuccess) hr = hipEventCreateWithFlags(&e->gathered_ev, hipEventDisableTiming);
        if (rc == BH_OK && hr != hipSuccess) {
            e->err = std::string("comm stream/events: ") + hipGetErrorString(hr);
            rc = BH_E_DEVICE;
        }
        // the accelerations buffer is laid out in rounds x world pieces from now on
        if (rc == BH_OK) {
            const int64_t cap = e->cap;
            e->cap = 0;
            rc = ensure_capacity(e, cap);
        }
        if (rc == BH_OK) rc = agree_settings(e);
    }
    if (rc != BH_OK) {
        std::fprintf(stderr, "bh_create_dist: %s\n", e->err.c_str());
        bh_destroy(e);
        return rc;
    }
    *out = e;
    return BH_OK;
}

int bh_local_group_create(int world, bh_local_group **out) {
    if (!out || world < 1) return BH_E_INVALID;
    bh_local_group *g = new bh_local_group();
    g->world = world;
    g->members.assign((size_t)world, nullptr);
    *out = g;
    return BH_OK;
}

void bh_local_group_destroy(bh_local_group *g) { delete g; }

int bh_create_local(const bh_params *p, int device, int rank, bh_local_group *group,
                    bh_engine **out) {
    if (!out || !group || rank < 0 || rank >= group->world || group->members[rank])
        return BH_E_INVALID;
    *out = nullptr;
    bh_engine *e = new bh_engine();
    e->rank = rank;
    e->world = group->world;
    int rc = engine_init(e, p, device);
    if (rc == BH_OK) {
        hipError_t hr = comm_stream_create(&e->comm_stream);
        for (int k = 0; k < BH_SHARD_ROUNDS && hr == hipSuccess; ++k)
            hr = hipEventCreateWithFlags(&e->round_ev[k], hipEventDisableTiming);
        if (hr == hipSuccess) hr = hipEventCreateWithFlags(&e->gathered_ev, hipEventDisableTiming);
        if (hr != hipSuccess) {
            e->err = std::string("comm stream/events: ") + hipGetErrorString(hr);
            rc = BH_E_DEVICE;
        }
    }
    if (rc == BH_OK) {
        e->group = group;
        const int64_t cap = e->cap;  // the accelerations buffer in rounds x world pieces
        e->cap = 0;
        rc = ensure_capacity(e, cap);
    }
    if (rc != BH_OK) {
        std::fprintf(stderr, "bh_create_local: %s\n", e->err.c_str());
        e->group = nullptr;
        bh_destroy(e);
        return rc;
    }
    group->members[rank] = e;
    *out = e;
    return BH_OK;
}

int bh_create_solo(const bh_params *p, int device, int rank, int world, bh_engine **out) {
    if (!out || world < 1 || rank < 0 || rank >= world) return BH_E_INVALID;
    *out = nullptr;
    bh_engine *e = new bh_engine();
    e->rank = rank;
    e->world = world;
    int rc = engine_init(e, p, device);
    if (rc == BH_OK) {
        hipError_t hr = comm_stream_create(&e->comm_stream);
        for (int k = 0; k < BH_SHARD_ROUNDS && hr == hipSuccess; ++k)
            hr = hipEventCreateWithFlags(&e->round_ev[k], hipEventDisableTiming);
        if (hr == hipSuccess) hr = hipEventCreateWithFlags(&e->gathered_ev, hipEventDisableTiming);
        if (hr != hipSuccess) {
            e->err = std::string("comm stream/events: ") + hipGetErrorString(hr);
            rc = BH_E_DEVICE;
        }
    }
    if (rc == BH_OK) {
        e->solo = true;
        const int64_t cap = e->cap;  // the pieces buffer in rounds x world pieces
        e->cap = 0;
        rc = ensure_capacity(e, cap);
    }
    if (rc != BH_OK) {
        std::fprintf(stderr, "bh_create_solo: %s\n", e->err.c_str());
        bh_destroy(e);
        return rc;
    }
    *out = e;
    return BH_OK;
}

void bh_destroy(bh_engine *e) {
    if (!e) return;
    if (e->step_thr.joinable()) e->step_thr.join();  // a call begun by bh_step_begin
    if (e->multi) {  // the members, their threads and the exchange; then the handle itself
        bh_destroy(e->one);
        multi_destroy(e->multi);
        delete e;
        return;
    }
    (void)hipSetDevice(e->device);
    // (a rank of a decomposition waits for its streams at most BH_COMM_TIMEOUT_S: a collective
    // whose peers are gone never completes; after a failed call its communicator is aborted --
    // ncclCommDestroy would wait for the peers)
    const double drain_s = multi_rank(e) ? std::max(comm_timeout_s(), 1.0) : 0.0;
    if (e->comm && (e->comm_failed || peers_aborted(e))) abort_comm(e);
    (void)drain_stream(e->stream, drain_s);
    if (e->comm && drain_stream(e->comm_stream, drain_s) != hipSuccess) abort_comm(e);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    if (e->group && e->rank < (int)e->group->members.size() && e->group->members[e->rank] == e)
        e->group->members[e->rank] = nullptr;
    for (hipEvent_t ev : e->round_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->gathered_ev) (void)hipEventDestroy(e->gathered_ev);
    if (e->comm_stream) (void)hipStreamDestroy(e->comm_stream);
    if (e->stream2) {
        (void)hipStreamSynchronize(e->stream2);
        (void)hipStreamDestroy(e->stream2);
    }
    if (e->built_ev) (void)hipEventDestroy(e->built_ev);
    for (hipEvent_t ev : e->pipe_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->pipe_stream) {
        (void)hipStreamSynchronize(e->pipe_stream);
        (void)hipStreamDestroy(e->pipe_stream);
    }
    if (e->mir_stream) {
        (void)hipStreamSynchronize(e->mir_stream);
        (void)hipStreamDestroy(e->mir_stream);
    }
    for (hipEvent_t ev : {e->mir_ev, e->mir_ev2, e->mir_ev3, e->mir_in[0], e->mir_in[1], e->mid_ev,
                          e->mid_sv_ev})
        if (ev) (void)hipEventDestroy(ev);
    for (double *b : e->mir_buf)
        if (b) (void)hipHostFree(b);
    if (e->mir_idx) (void)hipHostFree(e->mir_idx);
    free_state(e->view);
    free_state(e->st);
    free_state(e->alt);
    free_state(e->snap);
    free_state(e->sub_src);
    free_state(e->sub_dst);
    if (e->sub_cnt_ev) (void)hipEventDestroy(e->sub_cnt_ev);
    if (e->sub_cnt_h) (void)hipHostFree(e->sub_cnt_h);
    if (e->table_ev) (void)hipEventDestroy(e->table_ev);
    void *lets[] = {e->L.own_blk, e->L.rowmask, e->let_box, e->disp, e->inv_lanes, e->L.csrc, e->L.ccnt, e->L.cpos, e->solo_table, e->solo_all, e->solo_cstart, e->L.ecell, e->L.hcell, e->L.own, e->L.subpos, e->L.flag_all, e->L.flag8, e->L.sel, e->L.selpos, e->L.cstart,
                    e->L.table, e->L.tables, e->L.levels, e->L.w, e->L.posc, e->L.bsz,
                    e->L.nodes, e->L.lanes, e->s_keys, e->s_keys_s, e->s_spl, e->s_keys32,
                    e->s_keys32_s, e->s_idx, e->s_perm, e->s_cpl, e->s_cnt, e->s_base,
                    e->s_cell_start, e->s_span_list, e->s_super_list, e->s_bcount, e->s_bstart,
                    e->s_span_children, e->s_nodes};
    for (void *q : lets)
        if (q) (void)hipFree(q);
    void *ptrs[] = {e->a2, e->ax, e->ay, e->keys, e->keys_s, e->keys32, e->keys32_s, e->idx, e->perm, e->perm2, e->cpl, e->cnt,
                    e->base, e->cell_start, e->nodes, e->span_list, e->super_list,
                    e->span_children, e->scalars, e->visits32, e->contrib32, e->lanes, e->wave_iters, e->wave_blocks, e->heavy, e->keep,
                    e->pos, e->box, e->dlog, e->dead_sorted, e->rkeys, e->ridx, e->mbits, e->mslot, e->scratch,
                    e->leaf_flags, e->leaf_sel, e->leaf_count, e->leaf_cover, e->leaves.rec,
                    e->leaf_tmp, e->spl, e->bcount, e->bstart, e->nodes_alt, e->wave_cost, e->run_order,
                    e->m_trav, e->cidx_trav, e->lanes_trav, e->T_trav, e->solo_xchg,
                    e->lt_x, e->lt_y, e->lt_keys, e->lt_cpl, e->lt_base, e->mir_stage,
                    e->mir_keep, e->mir_pos, e->mir_tmp, e->mir_idx_stage, e->lanes_next, e->lr_hkey, e->lr_hkey_s,
                    e->lr_slot, e->lr_scratch, e->phi, e->diag_part, e->rnd_packed, e->rnd_cnt,
                    e->rnd_pixels, e->rnd_owner, e->rnd_counts, e->qd_rowd, e->qd_cold, e->qd_dir,
                    e->qd_out, e->qd_count, e->fld_in, e->fld_out, e->fld_u32, e->fld_scratch,
                    e->dfl_in, e->dfl_out, e->dfl_u32, e->dfl_slot_of, e->fgr_out, e->fgr_stats,
                    e->nbr_in, e->nbr_u32, e->nbr_i64, e->nbr_d2, e->nbr_scratch, e->nbr_idx,
                    e->nbr_list, e->nbr_sort, e->knn_in, e->knn_u32, e->knn_scratch, e->knn_seed,
                    e->knn_found, e->knn_idx, e->knn_d2,
                    e->grp_u32, e->grp_u64, e->grp_i64, e->grp_part, e->grp_groups, e->grp_scratch,
                    e->rad_u32, e->rad_flag, e->rad_f64, e->rad_bins, e->rad_sub, e->rad_scratch,
                    e->trc, e->trc_snap, e->trc_u32, e->trc_scratch, e->slog_ring, e->slog_phi,
                    e->slog_stage, e->slog_part, e->slog_keep, e->slog_pos, e->slog_tmp};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    for (Stopwatch *sw : {&e->pot_sw, &e->fld_sw, &e->dfl_sw, &e->fgr_sw, &e->nbr_sw, &e->knn_sw, &e->grp_sw,
                          &e->grp_sw_run, &e->rad_sw, &e->rnd_sw, &e->qd_sw})
        sw->destroy();
    for (hipEvent_t ev : e->ev) (void)hipEventDestroy(ev);
    if (e->lr_ev) (void)hipEventDestroy(e->lr_ev);
    if (e->pin) (void)hipHostFree(e->pin);
    if (e->rnd_pin) (void)hipHostFree(e->rnd_pin);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// what the last call without a handle on this thread refused its arguments for
// (bh_field_grid_of_view; a static string, null after a success)
static thread_local const char *handleless_error = nullptr;

const char *bh_last_error(const bh_engine *e) {
    if (e) return e->err.c_str();
    return handleless_error ? handleless_error : "null engine";
}

int bh_set_params(bh_engine *e, const bh_params *p) {
    if (!e || !p) return BH_E_INVALID;
    ASYNC_GUARD(e);
    Geometry g;
    TRY(make_geometry(*p, g, e->err));
    if (e->multi) {
        e->p = *p;
        e->geo = g;
    }
    MULTI_BOTH(e, bh_set_params(m_, p));
    HIPCHK(e, hipSetDevice(e->device));
    const bool geo_changed = std::memcmp(&g, &e->geo, sizeof(g)) != 0;
    if (p->merge_max_mass != e->p.merge_max_mass || p->merge_min_dist != e->p.merge_min_dist)
        e->heavy_possible = true;
    e->p = *p;
    if (geo_changed) {
        TRY(materialize_positions(e));
        if (e->view_pending) {
            // the prebuilt tree (and its jitter) belong to the old root cell: back to the state the
            // caller sees, in its own slot order (the lane map described the prebuilt order)
            std::swap(e->st, e->view);
            e->view_pending = false;
            e->lanes_valid = e->lr_pending = e->lr_ready = false;
        }
        TRY(drop_carried_flags(e));
        e->prebuilt = false;
        e->lt_aside = false;
        e->boxes_valid = false;  // another grid
        e->geo = g;
        e->tree_valid = false;
        e->lazy_tree = false;
        e->spl_nb = 0;  // keys change meaning
        e->keys_ready = false;
        e->lanes_valid = e->lr_pending = e->lr_ready = false;
        e->inv_valid = false;
        if (g.J != e->J_alloc) {  // tree workspace sized for another depth; the state stays
            SYNC(e, e->stream);
            TRY(ensure_capacity(e, e->n));
        }
    }
    return BH_OK;
}

int bh_get_params(const bh_engine *e, bh_params *p) {
    if (!e || !p) return BH_E_INVALID;
    e = MULTI_M0(e);
    *p = e->p;
    return BH_OK;
}

int bh_reset_bodies(bh_engine *e, int64_t n, const double *x, const double *y, const double *vx,
                    const double *vy, const double *m) {
    if (!e || n < 0 || (n > 0 && (!x || !y || !vx || !vy || !m))) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (n >= (int64_t)NODE_BODY_MASK) {
        e->err = "too many bodies";
        return BH_E_INVALID;
    }
    if (e->multi) {  // resetBodies picks the engine for this body list (BHA:377's min(cores, n))
        const bool one = n < e->multi_min;
        if (one && !e->one) {
            bh_engine *m0 = multi_member(e->multi, 0);
            bh_engine *o = nullptr;
            const int rc = bh_create(&m0->p, m0->device, &o);
            if (rc != BH_OK) {
                e->err = "the single-GPU engine for a small body list could not be created";
                return rc;
            }
            if (m0->mirror_on) TRY(bh_set_mirror(o, m0->mir_nbuf));
            TRY(bh_set_profiling(o, m0->profiling ? 1 : 0));
            e->one = o;
        }
        e->use_one = one;
    }
    if (e->multi) TRY(multi_repair(e->multi, e));  // after a failed call: fresh communicators
    MULTI_ALL(e, bh_reset_bodies(m_, n, x, y, vx, vy, m));
    e->prog_api.store(++e->api_calls);
    HIPCHK(e, hipSetDevice(e->device));
    if (multi_rank(e) && (e->comm_failed || e->comm_lost || peers_aborted(e))) {
        // the way back from a failed call: every stream idle, the group's barriers usable again
        if (e->comm_lost) {
            e->err = "bh_reset_bodies: the RCCL communicator was aborted after a failed call; "
                     "create the engine anew";
            return BH_E_COMM;
        }
        for (hipStream_t s : {e->stream, e->stream2, e->comm_stream, e->pipe_stream, e->mir_stream})
            if (drain_stream(s, 30.0) != hipSuccess) {
                e->err = "bh_reset_bodies: a stream did not drain after the failed call";
                return BH_E_DEVICE;
            }
        e->comm_failed = false;
        e->fail_msg.clear();
        if (e->group) e->group->reset();
    }
    SYNC(e, e->stream);
    TRY(drop_carried_flags(e));
    e->vel_perm = nullptr;  // (the state is replaced)
    TRY(ensure_capacity(e, n));
    if (n > 0) {  // slot order = caller order until the first build
        HIPCHK(e, hipMemcpyAsync(e->st.x, x, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->st.y, y, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->st.vx, vx, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->st.vy, vy, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->st.m, m, sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
        iota_u32(e->st.cidx, n, e->stream);
        HIPCHK(e, hipGetLastError());
    }
    SYNC(e, e->stream);
    e->n = n;
    e->heavy_possible = true;
    e->removed.clear();
    e->slog_phi_valid = false;  // (the log itself runs on)
    e->tree_valid = false;  // BHA:348
    e->lazy_tree = false;
    e->prebuilt = false;    // other bodies: the pipelined call's next tree is void
    e->view_pending = false;
    e->lt_aside = false;
    e->mir_fresh = false;
    e->spl_nb = 0;          // other bodies: the first build sorts from scratch
    e->keys_ready = false;
    e->lanes_valid = e->lr_pending = e->lr_ready = false;
    e->st_morton = false;
    e->vel_stale = false;
    e->pos_pending = false;
    e->inv_valid = false;
    e->boxes_valid = false;
    return BH_OK;
}

static int step_call(bh_engine *e, int32_t k);
static int step_call_rank(bh_engine *e, int32_t k);

int bh_step(bh_engine *e, int32_t k) {
    if (!e || k < 0) return BH_E_INVALID;
    ASYNC_GUARD(e);
    return step_call(e, k);
}

// bh_step's work (bh_step_begin's thread calls it directly): a multi-device handle's members, or
// this engine's steps -- a rank of a decomposition refuses them after a failed call, and a call
// that fails on it aborts its peers' waits (fail_multi_rank)
static int step_call(bh_engine *e, int32_t k) {
    MULTI_ALL(e, bh_step(m_, k));  // every GPU's share of every step, joined (BHA:374-395, 408)
    COMM_GUARD(e);
    e->prog_busy.store(1);
    e->slog_call_head = e->slog_head;
    e->slog_call_step = e->slog_step;
    e->slog_call_t = e->slog_t;
    const int rc = fail_multi_rank(e, step_call_rank(e, k));
    if (rc != BH_OK) {  // a failed call leaves an empty log; step and t as before the call
        e->slog_head = 0;
        e->slog_step = e->slog_call_step;
        e->slog_t = e->slog_call_t;
        e->slog_phi_valid = false;
    }
    e->prog_busy.store(0);
    return rc;
}

static int step_call_rank(bh_engine *e, int32_t k) {
    e->prog_api.store(++e->api_calls);
    HIPCHK(e, hipSetDevice(e->device));
    e->trc_ms_sum = 0.0;  // bh_tracer_kernel_ms: this call's walks, timed only while profiling
    e->trc_launches = 0;
    e->slog_ms_sum = 0.0;  // bh_step_log_kernel_ms likewise
    e->slog_launches = 0;
    if (k > 0) TRY(step_log_bufs(e));
    const bool may_merge = k > 0 && e->n > 1 && e->p.merge_min_dist > 0.0 && e->heavy_possible;
    // a multi-rank call with LET builds may have to be replayed with a larger subset capacity
    const bool may_let = k > 0 && e->n > 0 && (e->comm || e->group || e->solo) && let_active(e) &&
                         !theta2_is_zero(e);
    if (may_merge || may_let) TRY(snapshot(e));
    // the previous call's pipelined last step built this call's first tree (a replay does not
    // use it: restore() starts from the caller-visible state)
    const bool carried = k > 0 && e->prebuilt;
    if (k > 0) {
        e->mir_fresh = false;
        e->lt_aside = false;  // lastTree will be this call's (nodes_alt is rebuilt below)
    }
    int let_replays = 0;
    for (bool first = true;; first = false) {
        e->ev_used = 0;
        e->timings_pending = false;
        if (!first && e->mid_armed) {  // a replay: an earlier attempt's hand-off is void
            std::lock_guard<std::mutex> lk(e->mid_mu);
            e->mid_void = true;
        }
        // the subset splitters are trusted only within a call (another scene after a reset
        // would put most of a subset into one bucket): the first LET build sorts with rocprim
        e->s_spl_nb = 0;
        HIPCHK(e, hipMemsetAsync(e->scalars + 1, 0, 5 * sizeof(uint32_t), e->stream));
        e->removed.clear();
        e->merge_ran = false;
        if (k > 0) e->prebuilt = first && carried;
        e->lazy_tree = false;
        e->mir_launched = false;
        for (int32_t s = 0; s < k; ++s) TRY(step_once(e, s + 1 == k));
        // a copy-out launched by the last pipelined step reads the state the compaction (or a
        // replay's restore) below rewrites
        if (e->mir_launched) HIPCHK(e, hipStreamWaitEvent(e->stream, e->mir_ev2, 0));
        // (one GPU: no wait here -- the merge bookkeeping's read-back below, or the tree flags'
        // when nothing merged, is queued behind the steps and waited for once)
        if (may_let) SYNC(e, e->stream);
        if (may_let) {  // LET subset sizes of this call: [4] some rank overflowed, [5] largest
            uint32_t ls[2] = {0, 0};
            // [4] can be set after the cell tables were exchanged (k_let_guard, k_let_w): on one
            // rank only.  Every rank must take the same decision, or one replays alone and issues
            // collectives its peers never match -- so the flags are max-reduced over the ranks.
            uint32_t own_sub = 0;
            TRY(agree_let_flags(e, ls, &own_sub));
            if (ls[1] > 0) {
                e->let_last_sub = own_sub;
                e->let_known = std::max<int64_t>(ls[1], ls[0] ? e->let_known : 1);
            }
            if (ls[0]) {  // every rank saw the overflow (exchanged): all replay the call
                // (the builds after an overflow saw a damaged state, so a replay can meet a
                // larger subset than observed; the third replay builds subsets of any size)
                if (++let_replays >= 3) e->let_known = e->n;
                ++e->let_overflows;
                e->removed.clear();
                e->merge_ran = false;
                TRY(restore(e));
                continue;
            }
        }
        // every replica complete at the API boundary: after a call that ended with a LET
        // evaluation the positions are in the exchange buffer and the peers' velocities with
        // their owners (every rank runs this: the velocity all-gather is collective)
        if (e->vel_stale && k > 0) {
            TRY(materialize_positions(e));
            TRY(sync_velocities(e));
        }
        // the merge bookkeeping first, so that an error below leaves a compacted state
        uint32_t overflow = 0, tflags = 0;
        bool have_flags = false;
        TRY(finish_merges(e, &overflow, &tflags, &have_flags));  // (reads the flags too)
        int tree_rc = BH_OK;
        if (e->n > 0 && k > 0) {
            if (!have_flags) {
                tree_rc = check_tree_flags(e);
            } else if (tflags) {
                e->err = "jitter replay reached an unsupported geometry (body stayed inside a "
                         "depth J+1 cell)";
                tree_rc = BH_E_STATE;
            }
        }
        if (overflow) {  // a step's candidate pairs exceeded the mailbox: replay the call
            if (!may_merge) {
                e->err = "merge rule: candidate mailbox overflow without a snapshot";
                return BH_E_STATE;
            }
            e->box_need = (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, 2ull * overflow);
            TRY(merge_bufs(e));
            TRY(restore(e));
            continue;
        }
        if (tree_rc != BH_OK) return tree_rc;
        break;
    }
    if (k > 0 && e->mirror_on) {
        if (!e->mir_launched)  // the call's last step was not pipelined: copy out now
            TRY(mirror_launch(e, e->view_pending ? e->view : e->st, e->stream, e->stream));
        // the next call reuses the buffers the mirror's kernels read (not its host copies)
        HIPCHK(e, hipStreamWaitEvent(e->stream, e->mir_ev2, 0));
        e->mir_fresh = true;
        e->mir_n = e->n;
    }
    if (e->profiling) TRY(collect_timings(e));
    return BH_OK;
}

int bh_step_begin(bh_engine *e, int32_t k) {
    if (!e || k < 0) return BH_E_INVALID;
    if (e->async_running) return BH_E_STATE;  // (its call may be writing the error text)
    bh_engine *t = MULTI_M0(e);  // the engine whose mirror the call fills
    if (!t->mirror_on || t->mir_nbuf != 2) {
        e->err = "bh_step_begin: needs the two-buffer mirror (bh_set_mirror(e, 2))";
        return BH_E_STATE;
    }
    if (e->step_thr.joinable()) e->step_thr.join();
    {
        std::lock_guard<std::mutex> lk(t->mid_mu);
        t->mid_armed = k > 0;
        t->mid_ready = t->mid_done = t->mid_void = false;
    }
    e->mid_eng = t;
    e->mid_n0 = t->n;
    e->mid_surv_done = false;
    e->async_rc = BH_OK;
    e->async_running = true;
    e->step_thr = std::thread([e, t, k] {
        const int rc = step_call(e, k);
        {
            std::lock_guard<std::mutex> lk(t->mid_mu);
            e->async_rc = rc;
            t->mid_armed = false;
            t->mid_done = true;
        }
        t->mid_cv.notify_all();
    });
    return BH_OK;
}

int bh_step_positions(bh_engine *e, const double **x, const double **y, const double **m,
                      const uint32_t **survivors, int64_t *n_out, int64_t *n_before) {
    if (!e) return BH_E_INVALID;
    if (!e->async_running || !e->mid_eng) {
        e->err = "bh_step_positions: no call begun (bh_step_begin)";
        return BH_E_STATE;
    }
    bh_engine *t = e->mid_eng;
    const double *buf = nullptr;
    int64_t stride = 0, n = 0;
    std::unique_lock<std::mutex> lk(t->mid_mu);
    t->mid_cv.wait(lk, [t] { return t->mid_ready || t->mid_done; });
    if (!t->mid_done && !t->mid_void) {  // the hand-off: usable unless the call will replay
        buf = t->mid_buf;
        stride = t->mid_stride;
        lk.unlock();
        // x, y, m not asked for: the survivors are enough (their copy runs ahead of the planes')
        HIPCHK(e, hipEventSynchronize(x || y || m ? t->mid_ev : t->mid_sv_ev));
        const uint32_t *h = t->mir_idx;  // scalars[1] tree flags, [2] removals, [3] overflow
        n = e->mid_n0 - (int64_t)h[2];
        lk.lock();
        if (h[1] || h[3] || t->mid_void) buf = nullptr;  // an error or a replay follows: the end
    }
    if (!buf) {  // no hand-off (a call whose last step is not pipelined, or a replay): the end
        t->mid_cv.wait(lk, [t] { return t->mid_done; });
        lk.unlock();
        if (e->async_rc != BH_OK) return e->async_rc;
        HIPCHK(e, hipEventSynchronize(t->mir_ev));
        buf = t->mir;
        stride = t->mir_cap;
        n = t->mir_n;
        if (!e->mid_surv_done) {  // the survivors from the call's removals: a mirror written
            // after the call's compaction numbers its bodies in the list after the call
            int64_t nr = 0;
            int rc = last_removed(e, nullptr, 0, &nr);
            if (rc != BH_OK && rc != BH_E_CAPACITY) return rc;
            std::vector<int64_t> rem((size_t)std::max<int64_t>(nr, 1));
            TRY(last_removed(e, rem.data(), nr, &nr));
            uint32_t *sv = t->mir_idx + MIRROR_HDR;
            int64_t j = 0, r = 0;
            for (int64_t i = 0; i < e->mid_n0; ++i) {
                if (r < nr && rem[(size_t)r] == i) {
                    ++r;
                    continue;
                }
                sv[j++] = (uint32_t)i;
            }
            if (j != n) {
                e->err = "bh_step_positions: the removals do not match the mirror";
                return BH_E_STATE;
            }
            e->mid_surv_done = true;
        }
    }
    if (x) *x = buf;
    if (y) *y = buf + stride;
    if (m) *m = buf + 4 * stride;
    if (survivors) *survivors = t->mir_idx + MIRROR_HDR;
    if (n_out) *n_out = n;
    if (n_before) *n_before = e->mid_n0;
    return BH_OK;
}

int bh_step_end(bh_engine *e) {
    if (!e) return BH_E_INVALID;
    if (!e->async_running) {
        e->err = "bh_step_end: no call begun (bh_step_begin)";
        return BH_E_STATE;
    }
    e->step_thr.join();
    e->async_running = false;
    e->mid_eng = nullptr;
    return e->async_rc;
}

int64_t bh_num_bodies(const bh_engine *e) {
    if (!e) return -1;
    if (e->async_running && std::this_thread::get_id() != e->step_thr.get_id())
        return -1;  // (a call begun by bh_step_begin writes n: ask after bh_step_end)
    return MULTI_M0(e)->n;
}

int bh_get_bodies(bh_engine *e, double *x, double *y, double *vx, double *vy, double *m,
                  int64_t cap, int64_t *n_out) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (e->multi) {  // every replica is complete at the API boundary: member 0's
        const int rc = bh_get_bodies(MULTI_M0(e), x, y, vx, vy, m, cap, n_out);
        if (rc != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc;
    }
    COMM_GUARD(e);  // (a failed call's replica is not the reference's state)
    if (n_out) *n_out = e->n;
    if (cap < e->n) return BH_E_CAPACITY;
    HIPCHK(e, hipSetDevice(e->device));
    TRY(materialize_positions(e));
    const int64_t n = e->n;
    if (n > 0) {  // back to caller (list) order, staged in the second state buffer
        const BodyState &s = e->view_pending ? e->view : e->st;  // (not the prebuilt tree's jitter)
        const double *src[5] = {s.x, s.y, s.vx, s.vy, s.m};
        double *stage[5] = {e->alt.x, e->alt.y, e->alt.vx, e->alt.vy, e->alt.m};
        scatter_to_caller(n, s.cidx, 5, src, stage, e->stream);
        HIPCHK(e, hipGetLastError());
        double *dst[5] = {x, y, vx, vy, m};
        for (int k = 0; k < 5; ++k)
            if (dst[k])
                HIPCHK(e, hipMemcpyAsync(dst[k], stage[k], sizeof(double) * n,
                                         hipMemcpyDeviceToHost, e->stream));
    }
    SYNC(e, e->stream);
    return BH_OK;
}

int bh_set_mirror(bh_engine *e, int enabled) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (enabled < 0 || enabled > 2) {
        e->err = "bh_set_mirror: enabled is 0, 1 or 2";
        return BH_E_INVALID;
    }
    // (member 0's replica fills the mirror; the others' bh_set_mirror only reserves its stream)
    MULTI_BOTH(e, r_ == 0 ? bh_set_mirror(m_, enabled) : BH_OK);
    HIPCHK(e, hipSetDevice(e->device));
    e->mirror_on = enabled != 0;
    if (e->mirror_on && enabled != e->mir_nbuf) {  // another buffer count: made anew
        if (e->mir_stream) SYNC(e, e->mir_stream);
        e->mir_nbuf = enabled;
        e->mir_cap = 0;
        e->mir_fresh = false;
    }
    if (e->mirror_on) TRY(mirror_alloc(e));
    return BH_OK;
}

int bh_map_bodies(bh_engine *e, const double **x, const double **y, const double **vx,
                  const double **vy, const double **m, int64_t *n_out) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (e->multi) {
        const int rc = bh_map_bodies(MULTI_M0(e), x, y, vx, vy, m, n_out);
        if (rc != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc;
    }
    COMM_GUARD(e);
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->mir_fresh || e->mir_cap < e->n) {  // not written by the last call: copy out now
        TRY(materialize_positions(e));
        e->mir_launched = false;
        TRY(mirror_launch(e, e->view_pending ? e->view : e->st, e->stream, e->stream));
        HIPCHK(e, hipStreamWaitEvent(e->stream, e->mir_ev2, 0));
        e->mir_fresh = true;
        e->mir_n = e->n;
    }
    HIPCHK(e, hipEventSynchronize(e->mir_ev));
    const int64_t c = e->mir_cap;
    const double *b = e->mir;
    e->mir_front = b == e->mir_buf[1] ? 1 : 0;
    if (x) *x = b;
    if (y) *y = b + c;
    if (vx) *vx = b + 2 * c;
    if (vy) *vy = b + 3 * c;
    if (m) *m = b + 4 * c;
    if (n_out) *n_out = e->mir_n;
    return BH_OK;
}

static int compute_accelerations_rank(bh_engine *e, double *ax, double *ay, int64_t *visits);

int bh_compute_accelerations(bh_engine *e, double *ax, double *ay, int64_t *visits) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    // (every member builds and evaluates -- the build may jitter every replica alike; member 0
    // hands the results out)
    if (e->multi) {  // (the visit-counting walk is not sharded: every member counts)
        std::vector<std::vector<int64_t>> vis((size_t)multi_world(e->multi));
        const int64_t nb = bh_num_bodies(e);
        if (visits)
            for (size_t r = 1; r < vis.size(); ++r) vis[r].resize((size_t)std::max<int64_t>(nb, 1));
        MULTI_ALL(e, bh_compute_accelerations(m_, r_ == 0 ? ax : nullptr, r_ == 0 ? ay : nullptr,
                                              !visits ? nullptr
                                                      : r_ == 0 ? visits : vis[(size_t)r_].data()));
    }
    COMM_GUARD(e);
    return fail_multi_rank(e, compute_accelerations_rank(e, ax, ay, visits));
}

static int compute_accelerations_rank(bh_engine *e, double *ax, double *ay, int64_t *visits) {
    TRY(query_begin(e));
    const int64_t n = e->n;
    if (n == 0) return query_end(e, false);
    TRY(evaluate(e, visits ? e->visits32 : nullptr));
    scatter_acc_to_caller(n, e->st.cidx, e->a2, e->ax, e->ay, e->stream, e->a2_lanes,
                          e->a2_layout);
    HIPCHK(e, hipGetLastError());
    TRY(query_end(e, true));
    if (ax) HIPCHK(e, hipMemcpy(ax, e->ax, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (ay) HIPCHK(e, hipMemcpy(ay, e->ay, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (visits) {
        std::vector<uint32_t> v((size_t)n), c((size_t)n);
        HIPCHK(e, hipMemcpy(v.data(), e->visits32, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(c.data(), e->st.cidx, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        int64_t lane_sum = 0;
        for (int64_t i = 0; i < n; ++i) {
            visits[c[(size_t)i]] = v[(size_t)i];
            lane_sum += v[(size_t)i];
        }
        HIPCHK(e, hipMemcpy(v.data(), e->contrib32, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        int64_t contrib_sum = 0;
        for (int64_t i = 0; i < n; ++i) contrib_sum += v[(size_t)i];
        const int64_t waves = (n + 63) / 64;
        std::vector<uint32_t> wi((size_t)waves), wb((size_t)waves);
        HIPCHK(e, hipMemcpy(wi.data(), e->wave_iters, sizeof(uint32_t) * waves,
                            hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(wb.data(), e->wave_blocks, sizeof(uint32_t) * waves,
                            hipMemcpyDeviceToHost));
        int64_t wsum = 0, bsum = 0;
        for (uint32_t w : wi) wsum += w;
        for (uint32_t w : wb) bsum += w;
        e->stat_lane_visits = lane_sum;
        e->stat_lane_contrib = contrib_sum;
        e->stat_wave_iters = wsum;
        e->stat_wave_blocks = bsum;
        e->stat_waves = waves;
    }
    return BH_OK;
}

// The global sums over the state the caller sees, staged in the caller's list order (as
// bh_get_bodies stages it) so that the fixed-order reductions depend on the list alone; with_phi:
// e->phi (slot order, of the build the state is in) enters as sum m phi.
static int diagnostics_state(bh_engine *e, bool with_phi, bh_diagnostics *out) {
    *out = bh_diagnostics{};
    HIPCHK(e, hipSetDevice(e->device));
    const int64_t n = e->n;
    out->n = n;
    if (n <= 0) return BH_OK;
    TRY(potential_bufs(e));
    TRY(materialize_positions(e));
    const BodyState &s = e->view_pending ? e->view : e->st;
    const double *src[5] = {s.x, s.y, s.vx, s.vy, s.m};
    double *stage[5] = {e->alt.x, e->alt.y, e->alt.vx, e->alt.vy, e->alt.m};
    scatter_to_caller(n, s.cidx, 5, src, stage, e->stream);
    if (with_phi) {
        const double *ps[1] = {e->phi};
        double *pd[1] = {e->ax};
        scatter_to_caller(n, s.cidx, 1, ps, pd, e->stream);
    }
    double *res = e->diag_part + diag_partial_doubles() - 8;
    diag_reduce(n, e->alt.x, e->alt.y, e->alt.vx, e->alt.vy, e->alt.m, with_phi ? e->ax : nullptr,
                e->diag_part, res, e->stream);
    HIPCHK(e, hipGetLastError());
    double h[8];
    HIPCHK(e, hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    SYNC(e, e->stream);
    out->mass = h[0];
    out->mx = h[1];
    out->my = h[2];
    out->px = h[3];
    out->py = h[4];
    out->lz = h[5];
    out->kinetic = h[6];
    out->potential = with_phi ? 0.5 * h[7] : 0.0;
    return BH_OK;
}

// bh_compute_potential / bh_compute_diagnostics(with_potential) on one engine, state semantics of
// compute_accelerations_rank.  run: this engine evaluates and answers (else it only builds); phi
// (nullable): caller-order copy-out; diag (nullable): the reductions on the state after the build.
static int potential_rank(bh_engine *e, bool run, double *phi, bh_diagnostics *diag) {
    TRY(query_begin(e));
    const int64_t n = e->n;
    if (n > 0) {
        TRY(ensure_tree(e));
        if (run) TRY(potential_launch(e));
        if (run && phi) {
            const double *ps[1] = {e->phi};
            double *pd[1] = {e->ax};
            scatter_to_caller(n, e->st.cidx, 1, ps, pd, e->stream);
            HIPCHK(e, hipGetLastError());
        }
    }
    TRY(query_end(e, n > 0));
    if (run && phi && n > 0)
        HIPCHK(e, hipMemcpy(phi, e->ax, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (run && diag) TRY(diagnostics_state(e, n > 0, diag));
    return BH_OK;
}

int bh_compute_potential(bh_engine *e, double *phi) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    return query_call(e, [&](bh_engine *m, bool run) {
        return potential_rank(m, run, phi, nullptr);
    });
}

int bh_compute_diagnostics(bh_engine *e, int with_potential, bh_diagnostics *out) {
    if (!e || !out) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (with_potential)
        return query_call(e, [&](bh_engine *m, bool run) {
            return potential_rank(m, run, nullptr, out);
        });
    if (e->multi) {  // reductions only: member 0's replica (complete at the API boundary)
        const int rc = bh_compute_diagnostics(MULTI_M0(e), 0, out);
        if (rc != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc;
    }
    COMM_GUARD(e);
    return diagnostics_state(e, false, out);
}

// bh_*_kernel_ms of the stopwatch `sw`: the active engine's member 0 launched it.
static int kernel_ms(const bh_engine *e, Stopwatch bh_engine::*sw, double *ms) {
    if (!e || !ms) return BH_E_INVALID;
    return (MULTI_M0(e)->*sw).ms(ms);
}

int bh_potential_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::pot_sw, ms);
}

// A field query on one engine, state semantics of compute_accelerations_rank.  run: this engine
// evaluates by launch(tree) (else it only builds); the caller then copies the results out.
static int field_rank(bh_engine *e, bool run, const std::function<int(bool)> &launch) {
    TRY(query_begin(e));
    const bool tree = e->n > 0;
    if (tree) TRY(ensure_tree(e));
    if (run) TRY(launch(tree));
    if (run && !tree) SYNC(e, e->stream);  // no bodies, no tree: every sum stays +0.0
    return query_end(e, tree);
}

// The planes of P results at `res`, stride `cap`, to ax, ay, phi (each nullable).
static int field_copy_out(bh_engine *e, const double *res, int64_t cap, int64_t P, double *ax,
                          double *ay, double *phi) {
    double *out[3] = {ax, ay, phi};
    for (int k = 0; k < 3; ++k)
        if (out[k])
            HIPCHK(e, hipMemcpy(out[k], res + k * (size_t)cap, sizeof(double) * (size_t)P,
                                hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_compute_field(bh_engine *e, int64_t n_probe, const double *px, const double *py,
                     const double *pm, double *ax, double *ay, double *phi) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    TRY(check_list(e, "bh_compute_field", "n_probe", n_probe, px && py, "px or py"));
    const Probes p{n_probe, px, py, pm};
    return query_call(e, [&](bh_engine *m, bool run) {
        if (p.n == 0) run = false;
        TRY(field_rank(m, run, [&](bool tree) { return field_launch(m, p, tree); }));
        return run ? field_copy_out(m, m->fld_out, m->fld_cap, p.n, ax, ay, phi) : BH_OK;
    });
}

int bh_field_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::fld_sw, ms);
}

int bh_find_neighbors(bh_engine *e, int64_t n_probe, const double *px, const double *py, double r,
                      const double *pr, int64_t *count, int64_t *nearest, double *d2_nearest,
                      int64_t *offsets, int64_t *indices, int64_t cap, int64_t *n_total) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    TRY(check_list(e, "bh_find_neighbors", "n_probe", n_probe, px && py, "px or py"));
    const char *bad = nullptr;
    if (!pr && !(r >= 0.0)) bad = "r must be >= 0";
    else if ((offsets != nullptr) != (indices != nullptr)) bad = "offsets or indices is NULL";
    else if (cap < 0) bad = "cap must be >= 0";
    if (bad) {
        e->err = std::string("bh_find_neighbors: ") + bad;
        return BH_E_INVALID;
    }
    NeighborQuery q{n_probe, px, py, pr, r, false, nearest || d2_nearest, offsets != nullptr, cap};
    q.counting = count || q.lists || n_total || !q.nearest;
    TRY(query_call(e, [&](bh_engine *m, bool run) {
        if (q.n == 0) run = false;
        TRY(field_rank(m, run, [&](bool tree) { return neighbors_launch(m, q, tree); }));
        if (!run) return BH_OK;
        const NeighborPlanes pl = neighbor_planes(m);
        const size_t P = (size_t)q.n;
        auto out = [&](void *dst, const void *src, size_t bytes) {
            if (dst && bytes) HIPCHK(m, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            return BH_OK;
        };
        TRY(out(count, pl.count, sizeof(int64_t) * P));
        TRY(out(nearest, pl.nearest, sizeof(int64_t) * P));
        TRY(out(d2_nearest, m->nbr_d2, sizeof(double) * P));
        TRY(out(offsets, pl.offsets, sizeof(int64_t) * (P + 1)));
        if (q.filled) TRY(out(indices, m->nbr_list, sizeof(int64_t) * (size_t)q.total));
        return BH_OK;
    }));
    if (q.n == 0 && offsets) offsets[0] = 0;
    if (n_total) *n_total = q.total;
    if (q.lists && !q.filled && q.n > 0) {
        e->err = "bh_find_neighbors: cap is below the total; *n_total and offsets hold it";
        return BH_E_CAPACITY;
    }
    return BH_OK;
}

int bh_neighbors_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::nbr_sw, ms);
}

// null if (k, r_max) are usable and n lists of k entries can be addressed, else what is wrong
static const char *knn_args_error(int64_t n, int32_t k, double r_max) {
    if (k < 1 || k > BH_KNN_MAX_K) return "k must be in 1..64";
    if (!(r_max >= 0.0)) return "r_max must be >= 0";
    if (n * (int64_t)k > (int64_t)INT32_MAX) return "more than 2^31 - 1 entries in all: ask in batches";
    return nullptr;
}

// The rows of the first n lanes of m's planes to the caller's arrays (each nullable).
static int knn_copy_out(bh_engine *m, int64_t n, int k, int64_t *idx, double *d2, int64_t *found) {
    const size_t rows = (size_t)n * (size_t)k;
    if (idx && rows)
        HIPCHK(m, hipMemcpy(idx, m->knn_idx, sizeof(int64_t) * rows, hipMemcpyDeviceToHost));
    if (d2 && rows)
        HIPCHK(m, hipMemcpy(d2, m->knn_d2, sizeof(double) * rows, hipMemcpyDeviceToHost));
    if (found && n)
        HIPCHK(m, hipMemcpy(found, m->knn_found, sizeof(int64_t) * (size_t)n,
                            hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_find_knn(bh_engine *e, int64_t n_probe, const double *px, const double *py, int32_t k,
                double r_max, int64_t *idx, double *d2, int64_t *found) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    TRY(check_list(e, "bh_find_knn", "n_probe", n_probe, px && py, "px or py"));
    if (const char *bad = knn_args_error(n_probe, k, r_max)) {
        e->err = std::string("bh_find_knn: ") + bad;
        return BH_E_INVALID;
    }
    KnnQuery q{n_probe, px, py, (int)k, r_max, false, idx != nullptr, d2 != nullptr,
               found != nullptr};
    return query_call(e, [&](bh_engine *m, bool run) {
        if (q.n == 0) run = false;
        TRY(field_rank(m, run, [&](bool tree) { return knn_launch(m, q, tree); }));
        return run ? knn_copy_out(m, q.n, q.k, idx, d2, found) : BH_OK;
    });
}

int bh_find_knn_bodies(bh_engine *e, int32_t k, double r_max, int64_t *idx, double *d2,
                       int64_t *found, int64_t rows_cap, int64_t *n_rows) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    const char *bad = knn_args_error(0, k, r_max);
    if (!bad && rows_cap < 0) bad = "rows_cap must be >= 0";
    if (bad) {
        e->err = std::string("bh_find_knn_bodies: ") + bad;
        return BH_E_INVALID;
    }
    int64_t N = 0;
    const char *refused = nullptr;  // why the walk was not launched
    TRY(query_call(e, [&](bh_engine *m, bool run) {
        KnnQuery q{0, nullptr, nullptr, (int)k, r_max, true, idx != nullptr, d2 != nullptr,
                   found != nullptr};
        TRY(field_rank(m, run, [&](bool tree) {
            N = m->n;
            if (N > rows_cap) return BH_OK;
            if ((refused = knn_args_error(N, k, r_max))) return BH_OK;
            return knn_launch(m, q, tree);
        }));
        if (!run || N > rows_cap || refused) return BH_OK;
        return knn_copy_out(m, N, q.k, idx, d2, found);
    }));
    if (n_rows) *n_rows = N;
    if (refused) {
        e->err = std::string("bh_find_knn_bodies: ") + refused;
        return BH_E_INVALID;
    }
    if (N > rows_cap) {
        e->err = "bh_find_knn_bodies: rows_cap is below the number of bodies; *n_rows holds it";
        return BH_E_CAPACITY;
    }
    return BH_OK;
}

int bh_knn_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::knn_sw, ms);
}

int bh_knn_shape(int64_t n_lane, int32_t k, int64_t *out4) {
    if (!out4 || n_lane < 0 || n_lane > ((int64_t)1 << 28) || k < 1 || k > BH_KNN_MAX_K)
        return BH_E_INVALID;
    const KnnShape sh = knn_shape(n_lane, k);
    out4[0] = sh.bpw;
    out4[1] = sh.wpb;
    out4[2] = sh.lds;
    out4[3] = sh.grid;
    return BH_OK;
}

int bh_find_groups(bh_engine *e, double link, int64_t min_members, int64_t *label,
                   int64_t label_cap, int64_t *members, int64_t members_cap, bh_group *groups,
                   int64_t groups_cap, bh_groups_summary *summary) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    const char *bad = nullptr;
    if (!(link >= 0.0)) bad = "link must be >= 0";
    else if (min_members < 1) bad = "min_members must be >= 1";
    else if (label_cap < 0) bad = "label_cap must be >= 0";
    else if (members_cap < 0) bad = "members_cap must be >= 0";
    else if (groups_cap < 0) bad = "groups_cap must be >= 0";
    if (bad) {
        e->err = std::string("bh_find_groups: ") + bad;
        return BH_E_INVALID;
    }
    bh_groups_summary sum{0, 0, 0, 0, -1, 0};
    const char *small = nullptr;  // the array whose cap is too small
    TRY(query_call(e, [&](bh_engine *m, bool run) {
        TRY(field_rank(m, run, [&](bool tree) {
            return tree ? groups_launch(m, link, min_members, sum) : BH_OK;
        }));
        if (!run || m->n == 0) return BH_OK;
        const int64_t N = m->n;
        if (label && label_cap < N) small = "label_cap is below the number of bodies";
        else if (members && members_cap < sum.n_in_tree) small = "members_cap is below n_in_tree";
        else if (groups && groups_cap < sum.n_groups) small = "groups_cap is below n_groups";
        if (small) return BH_OK;
        const GroupBufs B = group_bufs(m);
        auto out = [&](void *dst, const void *src, size_t bytes) {
            if (dst && bytes) HIPCHK(m, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            return BH_OK;
        };
        TRY(out(label, B.label, sizeof(int64_t) * (size_t)N));
        TRY(out(members, B.members, sizeof(int64_t) * (size_t)sum.n_in_tree));
        TRY(out(groups, B.groups, sizeof(bh_group) * (size_t)sum.n_groups));
        return BH_OK;
    }));
    if (summary) *summary = sum;
    if (small) {
        e->err = std::string("bh_find_groups: ") + small + "; summary holds the sizes";
        return BH_E_CAPACITY;
    }
    return BH_OK;
}

int bh_groups_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::grp_sw, ms);
}

// What bh_compute_radial_profile refuses its edges for (null: nothing).
static const char *radial_edges_error(int32_t n_bin, const double *edges) {
    if (!edges) return "edges is NULL";
    if (n_bin < 1 || n_bin > BH_RADIAL_MAX_BINS) return "n_bin must be in 1..BH_RADIAL_MAX_BINS";
    for (int32_t k = 0; k <= n_bin; ++k)
        if (std::isnan(edges[k])) return "an edge is NaN";
    if (edges[0] < 0.0) return "edges[0] must be >= 0";
    for (int32_t k = 0; k < n_bin; ++k)
        if (!(edges[k] < edges[k + 1])) return "edges must be strictly increasing";
    return nullptr;
}

// The planes of bh_compute_radial_profile's buffers for the engine's rad_cap.
static RadialBufs radial_bufs(const bh_engine *e) {
    const size_t cap = (size_t)e->rad_cap;
    RadialBufs B{};
    B.key = e->rad_u32;
    B.key_s = B.key + cap;
    B.val = B.key_s + cap;
    B.val_s = B.val + cap;
    B.start = B.val_s + cap;
    B.flag = e->rad_flag;
    B.terms = e->rad_f64;
    B.part = B.terms + 7 * cap;
    B.edges = B.part + 7 * radial_partial_slots(e->rad_cap);
    B.bins = e->rad_bins;
    B.scratch = e->rad_scratch;
    B.scratch_bytes = e->rad_scratch_bytes;
    return B;
}

// The caller-visible state (as diagnostics_state reads and stages it) binned: nothing of the
// state or of what the pipelined engine carries into the next call is written.  The arguments
// have been validated.
static int radial_state(bh_engine *e, double cx, double cy, double cvx, double cvy, int32_t n_bin,
                        const double *edges, const int64_t *subset, int64_t n_subset,
                        bh_radial_bin *bins, bh_radial_summary *summary) {
    const int64_t n = e->n;
    if (n <= 0 || (!bins && !summary)) {  // nothing to bin, or nothing asked for: no device work
        if (bins) std::memset(bins, 0, sizeof(bh_radial_bin) * (size_t)n_bin);
        if (summary) *summary = bh_radial_summary{};
        return BH_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (outgrown(e->rad_cap, e->rad_u32, n)) {
        const size_t cap = (size_t)n;
        TRY(dev_alloc(e, e->rad_u32, 4 * cap + BH_RADIAL_MAX_BINS + 5));
        TRY(dev_alloc(e, e->rad_flag, cap));
        TRY(dev_alloc(e, e->rad_f64,
                      7 * cap + 7 * radial_partial_slots(n) + BH_RADIAL_MAX_BINS + 1));
        TRY(dev_alloc(e, e->rad_bins, (size_t)BH_RADIAL_MAX_BINS));
        if (e->rad_scratch) (void)hipFree(e->rad_scratch);
        e->rad_scratch = nullptr;
        e->rad_scratch_bytes = radial_scratch_bytes(n);
        HIPCHK(e, hipMalloc(&e->rad_scratch, e->rad_scratch_bytes ? e->rad_scratch_bytes : 1));
        e->rad_cap = n;
    }
    if (subset && n_subset > 0 && outgrown(e->rad_sub_cap, e->rad_sub, n_subset)) {
        TRY(dev_alloc(e, e->rad_sub, (size_t)n_subset));
        e->rad_sub_cap = n_subset;
    }
    // (the planes are laid out for rad_cap; the kernels run over the first n entries of each)
    const RadialBufs B = radial_bufs(e);
    TRY(materialize_positions(e));
    HIPCHK(e, hipMemcpyAsync(B.edges, edges, sizeof(double) * ((size_t)n_bin + 1),
                             hipMemcpyHostToDevice, e->stream));
    if (subset && n_subset > 0)
        HIPCHK(e, hipMemcpyAsync(e->rad_sub, subset, sizeof(int64_t) * (size_t)n_subset,
                                 hipMemcpyHostToDevice, e->stream));
    const BodyState &s = e->view_pending ? e->view : e->st;  // (not the prebuilt tree's jitter)
    const double *src[5] = {s.x, s.y, s.vx, s.vy, s.m};
    double *stage[5] = {e->alt.x, e->alt.y, e->alt.vx, e->alt.vy, e->alt.m};
    TRY(e->rad_sw.start(e, e->stream));
    scatter_to_caller(n, s.cidx, 5, src, stage, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, radial_run(n, e->alt.x, e->alt.y, e->alt.vx, e->alt.vy, e->alt.m, cx, cy, cvx, cvy,
                         n_bin, subset != nullptr, e->rad_sub, subset ? n_subset : 0,
                         bins != nullptr, B, e->stream));
    TRY(e->rad_sw.stop(e, e->stream));
    uint32_t cls[5];  // where the four classes begin in the sorted keys, and n
    HIPCHK(e, hipMemcpyAsync(cls, B.start + n_bin, sizeof(cls), hipMemcpyDeviceToHost, e->stream));
    if (bins)
        HIPCHK(e, hipMemcpyAsync(bins, B.bins, sizeof(bh_radial_bin) * (size_t)n_bin,
                                 hipMemcpyDeviceToHost, e->stream));
    SYNC(e, e->stream);
    if (summary) {
        summary->n_bodies = n;
        summary->n_selected = (int64_t)cls[RADIAL_UNSELECTED];
        summary->n_binned = (int64_t)cls[RADIAL_INNER];
        summary->n_inner = (int64_t)(cls[RADIAL_OUTER] - cls[RADIAL_INNER]);
        summary->n_outer = (int64_t)(cls[RADIAL_NAN] - cls[RADIAL_OUTER]);
        summary->n_nan = (int64_t)(cls[RADIAL_UNSELECTED] - cls[RADIAL_NAN]);
    }
    return BH_OK;
}

int bh_compute_radial_profile(bh_engine *e, double cx, double cy, double cvx, double cvy,
                              int32_t n_bin, const double *edges, const int64_t *subset,
                              int64_t n_subset, bh_radial_bin *bins, bh_radial_summary *summary) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    const char *bad = radial_edges_error(n_bin, edges);
    if (!bad && subset) {
        const int64_t N = bh_num_bodies(e);
        if (n_subset < 0 || n_subset > ((int64_t)1 << 28)) bad = "n_subset must be in [0, 2^28]";
        for (int64_t j = 0; !bad && j < n_subset; ++j)
            if (subset[j] < 0 || subset[j] >= N) bad = "a subset index is outside [0, N)";
    }
    if (bad) {
        e->err = std::string("bh_compute_radial_profile: ") + bad;
        return BH_E_INVALID;
    }
    if (e->multi) {  // every replica is complete at the API boundary: member 0's
        const int rc = bh_compute_radial_profile(MULTI_M0(e), cx, cy, cvx, cvy, n_bin, edges,
                                                 subset, n_subset, bins, summary);
        if (rc != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc;
    }
    COMM_GUARD(e);
    return radial_state(e, cx, cy, cvx, cvy, n_bin, edges, subset, n_subset, bins, summary);
}

int bh_radial_profile_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::rad_sw, ms);
}

int bh_radial_edges(double r_min, double r_max, int32_t n_bin, int log_spacing, double *edges) {
    handleless_error = nullptr;
    const char *bad = nullptr;
    if (!edges) bad = "bh_radial_edges: edges is NULL";
    else if (n_bin < 1 || n_bin > BH_RADIAL_MAX_BINS)
        bad = "bh_radial_edges: n_bin must be in 1..BH_RADIAL_MAX_BINS";
    else if (!std::isfinite(r_min) || r_min < 0.0)
        bad = "bh_radial_edges: r_min must be finite and >= 0";
    else if (log_spacing && !(r_min > 0.0))
        bad = "bh_radial_edges: log spacing needs r_min > 0";
    else if (!std::isfinite(r_max) || !(r_max > r_min))
        bad = "bh_radial_edges: r_max must be finite and above r_min";
    if (bad) {
        handleless_error = bad;
        return BH_E_INVALID;
    }
    std::vector<double> out((size_t)n_bin + 1);
    const double span = log_spacing ? std::log2(r_max / r_min) : r_max - r_min;
    for (int32_t k = 1; k < n_bin; ++k)
        out[(size_t)k] = log_spacing ? r_min * std::exp2(span * (double)k / (double)n_bin)
                                     : r_min + span * ((double)k / (double)n_bin);
    out[0] = r_min;
    out[(size_t)n_bin] = r_max;
    for (int32_t k = 0; k < n_bin; ++k)
        if (!(out[(size_t)k] < out[(size_t)k + 1])) {
            handleless_error = "bh_radial_edges: the edges are not strictly increasing (bins "
                               "narrower than the spacing of binary64)";
            return BH_E_INVALID;
        }
    std::memcpy(edges, out.data(), sizeof(double) * out.size());
    return BH_OK;
}

int bh_neighbor_reach(const bh_params *p, int32_t depth, double *reach) {
    if (!p || !reach || depth < 0 || depth >= MAX_DEPTH_TAB) return BH_E_INVALID;
    Geometry g;
    std::string err;
    if (make_geometry(*p, g, err) != BH_OK) return BH_E_INVALID;
    *reach = neighbor_reach_at(neighbor_reach_terms(g), depth);
    return BH_OK;
}

int bh_compute_field_direct(bh_engine *e, int64_t n_probe, const double *px, const double *py,
                            const double *pm, double *ax, double *ay, double *phi) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    TRY(check_list(e, "bh_compute_field_direct", "n_probe", n_probe, px && py, "px or py"));
    const Probes p{n_probe, px, py, pm};
    return query_call(e, [&](bh_engine *m, bool run) {
        if (p.n == 0) run = false;
        TRY(field_rank(m, run, [&](bool tree) { return direct_field_launch(m, p, tree); }));
        return run ? field_copy_out(m, m->dfl_out, m->dfl_cap, p.n, ax, ay, phi) : BH_OK;
    });
}

// bh_compute_force_error's summary of the four sample arrays (include/bh_engine.h): sequential,
// in sample order, binary64, nothing contracted.
static void force_error_summary(int64_t k, const double *axt, const double *ayt, const double *axe,
                                const double *aye, bh_force_error *out) {
    *out = bh_force_error{};
    out->n_sample = k;
    out->worst = -1;
    double sum = 0.0, sumsq = 0.0;
    for (int64_t j = 0; j < k; ++j) {
        if (!(std::isfinite(axt[j]) && std::isfinite(ayt[j]) && std::isfinite(axe[j]) &&
              std::isfinite(aye[j])))
            continue;
        const double den = std::sqrt(axe[j] * axe[j] + aye[j] * aye[j]);
        if (!(den > 0.0)) continue;
        const double dx = axt[j] - axe[j], dy = ayt[j] - aye[j];
        const double rel = std::sqrt(dx * dx + dy * dy) / den;
        if (out->n_used == 0 || rel > out->max_rel) {  // the first on ties
            out->max_rel = rel;
            out->worst = j;
        }
        sum += rel;
        sumsq += rel * rel;
        ++out->n_used;
    }
    if (out->n_used > 0) {
        out->mean_rel = sum / (double)out->n_used;
        out->rms_rel = std::sqrt(sumsq / (double)out->n_used);
    }
}

// What bh_compute_force_error asks of the engine that answers.  idx: the validated caller indices.
struct ForceErrorArgs {
    int64_t k;
    const uint32_t *idx;
    double *axt, *ayt, *axe, *aye;
    bh_force_error *out;
};

// The samples' exact accelerations on the tree of the evaluation just enqueued, by
// k_direct_targets in body mode over the tree's leaf sequence; their tree accelerations (e->ax,
// e->ay by caller index) are gathered beside them.
static int force_error_launch(bh_engine *e, const ForceErrorArgs &fa) {
    const int64_t n = e->n, K = fa.k;
    const ForceParams fp = force_params(e);
    TRY(build_leaf_list(e));
    TRY(direct_field_bufs(e, K));
    if (outgrown(e->dfl_slot_cap, e->dfl_slot_of, n)) {
        TRY(dev_alloc(e, e->dfl_slot_of, (size_t)e->cap));
        e->dfl_slot_cap = e->cap;
    }
    const size_t cap = (size_t)e->dfl_cap;
    double *tx = e->dfl_in, *ty = tx + cap, *tm = ty + cap;
    uint32_t *idx = e->dfl_u32, *tslot = idx + cap;
    HIPCHK(e, hipMemcpyAsync(idx, fa.idx, sizeof(uint32_t) * (size_t)K, hipMemcpyHostToDevice,
                             e->stream));
    HIPCHK(e, direct_body_targets(n, e->st, idx, K, e->dfl_slot_of, e->ax, e->ay, tx, ty, tm, tslot,
                                  e->dfl_out + 3 * cap, e->dfl_out + 4 * cap, e->stream));
    TRY(e->dfl_sw.start(e, e->stream));
    direct_targets(e->leaves, e->leaf_count, tx, ty, tm, tslot, K, fp.G, fp.soft2, e->dfl_out,
                   e->dfl_out + cap, nullptr, e->stream);
    HIPCHK(e, hipGetLastError());
    return e->dfl_sw.stop(e, e->stream);
}

// compute_accelerations_rank's evaluation, then -- on the same tree, in the same call, run: by
// this engine -- force_error_launch and the answer (else the evaluation alone).
static int force_error_rank(bh_engine *e, bool run, const ForceErrorArgs &fa) {
    TRY(query_begin(e));
    const int64_t n = e->n, K = fa.k;
    const bool launch = run && K > 0 && n > 0;  // (K > 0 with n = 0 was refused: no valid index)
    if (n > 0) {
        TRY(evaluate(e, nullptr));
        scatter_acc_to_caller(n, e->st.cidx, e->a2, e->ax, e->ay, e->stream, e->a2_lanes,
                              e->a2_layout);
        HIPCHK(e, hipGetLastError());
        if (launch) TRY(force_error_launch(e, fa));
    }
    TRY(query_end(e, n > 0));
    if (!run) return BH_OK;
    std::vector<double> h((size_t)(4 * K));
    double *host[4] = {h.data(), h.data() + K, h.data() + 2 * K, h.data() + 3 * K};
    if (launch) {
        const size_t cap = (size_t)e->dfl_cap, bytes = sizeof(double) * (size_t)K;
        const int plane[4] = {3, 4, 0, 1};  // ax_tree, ay_tree, ax_exact, ay_exact
        for (int q = 0; q < 4; ++q)
            HIPCHK(e, hipMemcpy(host[q], e->dfl_out + plane[q] * cap, bytes,
                                hipMemcpyDeviceToHost));
    }
    double *user[4] = {fa.axt, fa.ayt, fa.axe, fa.aye};
    for (int q = 0; q < 4; ++q)
        if (user[q] && K > 0) std::memcpy(user[q], host[q], sizeof(double) * (size_t)K);
    if (fa.out) force_error_summary(K, host[0], host[1], host[2], host[3], fa.out);
    return BH_OK;
}

int bh_compute_force_error(bh_engine *e, int64_t n_sample, const int64_t *idx, double *ax_tree,
                           double *ay_tree, double *ax_exact, double *ay_exact,
                           bh_force_error *out) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    TRY(check_list(e, "bh_compute_force_error", "n_sample", n_sample, idx != nullptr, "idx"));
    const int64_t n = bh_num_bodies(e);
    std::vector<uint32_t> idx32((size_t)n_sample);
    for (int64_t j = 0; j < n_sample; ++j) {
        if (idx[j] < 0 || idx[j] >= n) {
            e->err = "bh_compute_force_error: idx[" + std::to_string(j) + "] = " +
                     std::to_string(idx[j]) + " is outside [0, " + std::to_string(n) + ")";
            return BH_E_INVALID;
        }
        idx32[(size_t)j] = (uint32_t)idx[j];
    }
    const ForceErrorArgs fa{n_sample, idx32.data(), ax_tree, ay_tree, ax_exact, ay_exact, out};
    // (every member evaluates as bh_compute_accelerations does; member 0 does the rest)
    return query_call(e, [&](bh_engine *m, bool run) { return force_error_rank(m, run, fa); });
}

int bh_direct_field_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::dfl_sw, ms);
}

int bh_direct_field_shape(int64_t n_target, int64_t *out3) {
    if (!out3 || n_target < 0) return BH_E_INVALID;
    const DirectFieldShape sh = direct_field_shape(n_target);
    out3[0] = sh.tile;
    out3[1] = sh.lanes;
    out3[2] = sh.per_lane;
    return BH_OK;
}

// null if the grid's shape is usable, else what is wrong with it (the bounds are the view's)
static const char *field_grid_dims_error(int32_t nx, int32_t ny) {
    if (nx < 1 || nx > VIEW_MAX_SIDE || ny < 1 || ny > VIEW_MAX_SIDE)
        return "nx and ny must be in 1..16384";
    if ((int64_t)nx * (int64_t)ny > VIEW_MAX_PIXELS)
        return "nx * ny must not exceed 1 << 24";
    return nullptr;
}

int bh_compute_field_grid(bh_engine *e, const bh_field_grid *g, double *ax, double *ay,
                          double *phi, bh_field_grid_stats *stats) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (!g) {
        e->err = "bh_compute_field_grid: g is NULL";
        return BH_E_INVALID;
    }
    if (const char *why = field_grid_dims_error(g->nx, g->ny)) {
        e->err = std::string("bh_compute_field_grid: ") + why;
        return BH_E_INVALID;
    }
    if (!std::isfinite(g->x0) || !std::isfinite(g->y0) || !std::isfinite(g->dx) ||
        !std::isfinite(g->dy)) {
        e->err = "bh_compute_field_grid: x0, y0, dx and dy must be finite";
        return BH_E_INVALID;
    }
    const bh_field_grid grid = *g;
    const unsigned planes = (ax ? 1u : 0u) | (ay ? 2u : 0u) | (phi ? 4u : 0u);
    return query_call(e, [&](bh_engine *m, bool run) {
        TRY(field_rank(m, run, [&](bool tree) {
            return field_grid_launch(m, grid, planes, stats != nullptr, tree);
        }));
        if (!run) return BH_OK;
        TRY(field_copy_out(m, m->fgr_out, m->fgr_cap, (int64_t)grid.nx * grid.ny, ax, ay, phi));
        if (stats)  // the planes are row-major; their summary is the last of the partials
            HIPCHK(m, hipMemcpy(stats, m->fgr_stats + field_grid_stat_partials() - 1,
                                sizeof(*stats), hipMemcpyDeviceToHost));
        return BH_OK;
    });
}

int bh_field_grid_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::fgr_sw, ms);
}

int bh_field_grid_shape(int32_t nx, int32_t ny, int64_t *out4) {
    if (!out4 || field_grid_dims_error(nx, ny)) return BH_E_INVALID;
    const FieldGridShape sh = field_grid_shape(nx, ny);
    out4[0] = sh.tile_w;
    out4[1] = sh.tile_h;
    out4[2] = sh.wpb;
    out4[3] = sh.tiles;
    return BH_OK;
}

int bh_field_grid_of_view(const bh_view *v, int32_t cell_px, bh_field_grid *g) {
    const char *why = nullptr;
    if (!v || !g)
        why = "bh_field_grid_of_view: v or g is NULL";
    else if ((why = view_error(*v)) == nullptr && (cell_px < 1 || cell_px > VIEW_MAX_SIDE))
        why = "bh_field_grid_of_view: cell_px must be in 1..16384";
    handleless_error = why;
    if (why) return BH_E_INVALID;
    const double cell = (double)cell_px;
    g->nx = (v->width + cell_px - 1) / cell_px;
    g->ny = (v->height + cell_px - 1) / cell_px;
    g->dx = g->dy = cell / v->zoom;
    g->x0 = v->view_x + (0.5 * cell) / v->zoom;
    g->y0 = v->view_y + (0.5 * cell) / v->zoom;
    return BH_OK;
}

// The caller-visible state rasterised (render.hip): reads x, y, m, cidx of `view_pending ? view :
// st` in slot order -- no scatter to caller order, nothing of the state or of what the pipelined
// engine carries into the next call is written -- into the engine's render buffers.
static int render_buffers(bh_engine *e, size_t pad, bool pixels, bool owner, bool counts) {
    if (pad != e->rnd_pad) {  // another view size: made anew
        void **all[] = {(void **)&e->rnd_packed, (void **)&e->rnd_cnt, (void **)&e->rnd_pixels,
                        (void **)&e->rnd_owner, (void **)&e->rnd_counts};
        for (void **q : all) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        e->rnd_pad = pad;
    }
    if (!e->rnd_packed) {
        TRY(dev_alloc(e, e->rnd_packed, pad));
        HIPCHK(e, hipMemsetAsync(e->rnd_packed, 0, sizeof(uint32_t) * pad, e->stream));
    }
    if (counts && !e->rnd_cnt) {
        TRY(dev_alloc(e, e->rnd_cnt, pad));
        HIPCHK(e, hipMemsetAsync(e->rnd_cnt, 0, sizeof(uint32_t) * pad, e->stream));
    }
    if (pixels && !e->rnd_pixels) TRY(dev_alloc(e, e->rnd_pixels, pad));
    if (owner && !e->rnd_owner) TRY(dev_alloc(e, e->rnd_owner, pad));
    if (counts && !e->rnd_counts) TRY(dev_alloc(e, e->rnd_counts, pad));
    if (!e->rnd_clean) {  // a call that failed between its two kernels left the planes as they were
        HIPCHK(e, hipMemsetAsync(e->rnd_packed, 0, sizeof(uint32_t) * pad, e->stream));
        if (e->rnd_cnt)
            HIPCHK(e, hipMemsetAsync(e->rnd_cnt, 0, sizeof(uint32_t) * pad, e->stream));
        e->rnd_clean = true;
    }
    return BH_OK;
}

static int render_state(bh_engine *e, const bh_view &v, uint8_t *pixels, uint32_t *owner,
                        uint32_t *counts) {
    const size_t npix = (size_t)v.width * (size_t)v.height;
    const int64_t n = e->n;
    if (n <= 0) {  // nothing drawn: no device work
        if (pixels) std::memset(pixels, 0, npix);
        if (owner) std::memset(owner, 0xFF, sizeof(uint32_t) * npix);
        if (counts) std::memset(counts, 0, sizeof(uint32_t) * npix);
        return BH_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    TRY(materialize_positions(e));
    const size_t pad = render_padded_pixels(v.width, v.height);
    TRY(render_buffers(e, pad, pixels != nullptr, owner != nullptr, counts != nullptr));
    const BodyState &s = e->view_pending ? e->view : e->st;  // (not the prebuilt tree's jitter)
    e->rnd_clean = false;
    TRY(e->rnd_sw.start(e, e->stream));
    render_raster(n, s.x, s.y, s.m, s.cidx, v, e->rnd_packed, counts ? e->rnd_cnt : nullptr,
                  e->stream);
    HIPCHK(e, hipGetLastError());
    render_resolve(pad, e->rnd_packed, counts ? e->rnd_cnt : nullptr,
                   pixels ? e->rnd_pixels : nullptr, owner ? e->rnd_owner : nullptr,
                   counts ? e->rnd_counts : nullptr, e->stream);
    HIPCHK(e, hipGetLastError());
    TRY(e->rnd_sw.stop(e, e->stream));
    e->rnd_clean = true;
    // BH_RENDER_PINNED=1: through a pinned bounce buffer and a host copy (A/B, read per call)
    const char *env = std::getenv("BH_RENDER_PINNED");
    const bool pinned = env && std::atoi(env) != 0;
    void *dst[3] = {pixels, owner, counts};
    const void *src[3] = {e->rnd_pixels, e->rnd_owner, e->rnd_counts};
    const size_t bytes[3] = {npix, sizeof(uint32_t) * npix, sizeof(uint32_t) * npix};
    if (pinned && e->rnd_pin_bytes < 9 * npix) {
        if (e->rnd_pin) (void)hipHostFree(e->rnd_pin);
        e->rnd_pin = nullptr;
        e->rnd_pin_bytes = 0;
        HIPCHK(e, hipHostMalloc((void **)&e->rnd_pin, 9 * npix, hipHostMallocDefault));
        e->rnd_pin_bytes = 9 * npix;
    }
    size_t off = 0;
    for (int k = 0; k < 3; ++k) {
        if (!dst[k]) continue;
        HIPCHK(e, hipMemcpyAsync(pinned ? (void *)(e->rnd_pin + off) : dst[k], src[k], bytes[k],
                                 hipMemcpyDeviceToHost, e->stream));
        off += bytes[k];
    }
    SYNC(e, e->stream);
    if (pinned) {
        off = 0;
        for (int k = 0; k < 3; ++k) {
            if (!dst[k]) continue;
            std::memcpy(dst[k], e->rnd_pin + off, bytes[k]);
            off += bytes[k];
        }
    }
    return BH_OK;
}

void bh_default_view(bh_view *v) {
    if (v) view_defaults(v);
}

int bh_render_bodies(bh_engine *e, const bh_view *v, uint8_t *pixels, uint32_t *owner,
                     uint32_t *counts) {
    if (!e || !v) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (const char *why = view_error(*v)) {
        e->err = why;
        return BH_E_INVALID;
    }
    if (e->multi) {  // every replica is complete at the API boundary: member 0's
        const int rc = bh_render_bodies(MULTI_M0(e), v, pixels, owner, counts);
        if (rc != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc;
    }
    COMM_GUARD(e);
    return render_state(e, *v, pixels, owner, counts);
}

int bh_render_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::rnd_sw, ms);
}

int bh_set_tracers(bh_engine *e, int64_t n, const double *x, const double *y, const double *vx,
                   const double *vy) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    TRY(check_list(e, "bh_set_tracers", "n", n, x && y, "x or y"));
    if (e->multi || e->comm || e->group || e->solo) {
        if (n == 0) return BH_OK;  // (such an engine never holds tracers)
        e->err = "bh_set_tracers: tracers need the one-GPU engine (bh_create): this engine's steps "
                 "shard their builds as locally essential trees, which a tracer cannot walk";
        return BH_E_STATE;
    }
    HIPCHK(e, hipSetDevice(e->device));
    SYNC(e, e->stream);
    if (n != e->trc_n) {  // another count: every buffer anew, the lane map with them
        tracer_free(e);
        if (n == 0) return BH_OK;
        const size_t cap = (size_t)n;
        TRY(dev_alloc(e, e->trc, 4 * cap));
        TRY(dev_alloc(e, e->trc_u32, 4 * cap));
        e->trc_scratch_bytes = field_sort_bytes(n);
        HIPCHK(e, hipMalloc(&e->trc_scratch, e->trc_scratch_bytes ? e->trc_scratch_bytes : 1));
        e->trc_n = n;
    }
    if (n == 0) return BH_OK;
    const size_t s = (size_t)n, bytes = sizeof(double) * s;
    const double *src[4] = {x, y, vx, vy};
    for (int k = 0; k < 4; ++k) {
        if (src[k])
            HIPCHK(e, hipMemcpyAsync(e->trc + k * s, src[k], bytes, hipMemcpyHostToDevice,
                                     e->stream));
        else  // (all-zero bytes: +0.0)
            HIPCHK(e, hipMemsetAsync(e->trc + k * s, 0, bytes, e->stream));
    }
    TRY(tracer_reorder(e));
    SYNC(e, e->stream);
    return BH_OK;
}

int64_t bh_num_tracers(const bh_engine *e) {
    if (!e) return -1;
    return e->trc_n;  // (a multi-device handle holds none)
}

int bh_get_tracers(bh_engine *e, double *x, double *y, double *vx, double *vy, int64_t cap,
                   int64_t *n_out) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    const int64_t n = e->trc_n;
    if (n_out) *n_out = n;
    if (cap < n) return BH_E_CAPACITY;
    if (n == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    double *dst[4] = {x, y, vx, vy};
    for (int k = 0; k < 4; ++k)
        if (dst[k])
            HIPCHK(e, hipMemcpyAsync(dst[k], e->trc + k * (size_t)n, sizeof(double) * (size_t)n,
                                     hipMemcpyDeviceToHost, e->stream));
    SYNC(e, e->stream);
    return BH_OK;
}

int bh_tracer_kernel_ms(const bh_engine *e, double *avg_ms, int64_t *launches) {
    if (!e || !avg_ms) return BH_E_INVALID;
    if (e->async_running && std::this_thread::get_id() != e->step_thr.get_id()) return BH_E_STATE;
    *avg_ms = e->trc_launches ? e->trc_ms_sum / (double)e->trc_launches : 0.0;
    if (launches) *launches = e->trc_launches;
    return BH_OK;
}

int bh_set_step_log(bh_engine *e, int64_t capacity) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (capacity < 0 || capacity > ((int64_t)1 << 20)) {
        e->err = "bh_set_step_log: capacity must be in [0, 2^20]";
        return BH_E_INVALID;
    }
    if (e->multi || e->comm || e->group || e->solo) {
        if (capacity == 0) return BH_OK;  // (such an engine never holds a log)
        e->err = "bh_set_step_log: the step log needs the one-GPU engine (bh_create): this engine's "
                 "steps shard their builds as locally essential trees, which are not full trees -- "
                 "no walk of one gives a body its full potential";
        return BH_E_STATE;
    }
    HIPCHK(e, hipSetDevice(e->device));
    SYNC(e, e->stream);
    step_log_free(e, true);
    e->slog_head = e->slog_step = 0;
    e->slog_t = 0.0;
    if (capacity == 0) return BH_OK;
    HIPCHK(e, hipMalloc(&e->slog_ring, sizeof(bh_step_record) * (size_t)capacity));
    e->slog_cap = capacity;
    return BH_OK;
}

int bh_get_step_log(bh_engine *e, bh_step_record *out, int64_t cap, int64_t *n_out) {
    if (!e || !n_out || (!out && cap > 0)) return BH_E_INVALID;
    ASYNC_GUARD(e);
    const int64_t n = std::min(e->slog_head, e->slog_cap);
    *n_out = n;
    if (cap < n) return BH_E_CAPACITY;
    if (n == 0) return BH_OK;
    HIPCHK(e, hipSetDevice(e->device));
    SYNC(e, e->stream);
    // oldest first: the ring's tail from the next slot to write, then its head
    const bh_step_record *ring = static_cast<const bh_step_record *>(e->slog_ring);
    const int64_t first = e->slog_head > e->slog_cap ? e->slog_head % e->slog_cap : 0;
    const int64_t a = std::min(n, e->slog_cap - first);
    HIPCHK(e, hipMemcpy(out, ring + first, sizeof(bh_step_record) * (size_t)a,
                        hipMemcpyDeviceToHost));
    if (n > a)
        HIPCHK(e, hipMemcpy(out + a, ring, sizeof(bh_step_record) * (size_t)(n - a),
                            hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_get_step_log_phi(bh_engine *e, double *phi, int64_t cap, int64_t *n_out) {
    if (!e || !n_out || (!phi && cap > 0)) return BH_E_INVALID;
    ASYNC_GUARD(e);
    *n_out = 0;
    if (e->slog_cap <= 0) return BH_OK;  // no log: nothing to return
    if (!e->slog_phi_valid || e->slog_head <= 0) {
        e->err = "bh_get_step_log_phi: no step was logged since the log was enabled or the bodies "
                 "were replaced";
        return BH_E_STATE;
    }
    HIPCHK(e, hipSetDevice(e->device));
    SYNC(e, e->stream);
    const bh_step_record *ring = static_cast<const bh_step_record *>(e->slog_ring);
    bh_step_record last{};
    HIPCHK(e, hipMemcpy(&last, ring + (e->slog_head - 1) % e->slog_cap, sizeof(last),
                        hipMemcpyDeviceToHost));
    const int64_t n = last.d.n;
    if (n < 0 || n > e->slog_bcap) {
        e->err = "bh_get_step_log_phi: the last record's body count is out of range";
        return BH_E_STATE;
    }
    *n_out = n;
    if (cap < n) return BH_E_CAPACITY;
    if (n > 0)
        HIPCHK(e, hipMemcpy(phi, e->slog_stage + 5 * (size_t)e->slog_bcap,
                            sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_step_log_kernel_ms(const bh_engine *e, double *avg_ms, int64_t *launches) {
    if (!e || !avg_ms) return BH_E_INVALID;
    if (e->async_running && std::this_thread::get_id() != e->step_thr.get_id()) return BH_E_STATE;
    *avg_ms = e->slog_launches ? e->slog_ms_sum / (double)e->slog_launches : 0.0;
    if (launches) *launches = e->slog_launches;
    return BH_OK;
}

int bh_tracer_launch_shape(int64_t n_tracer, int64_t *out3) {
    if (!out3 || n_tracer < 0 || n_tracer > ((int64_t)1 << 28)) return BH_E_INVALID;
    const TracerShape sh = tracer_shape(n_tracer);
    out3[0] = sh.bpw;
    out3[1] = sh.wpb;
    out3[2] = sh.reorder;
    return BH_OK;
}

int bh_render_tracers(bh_engine *e, const bh_view *v, uint32_t *owner, uint32_t *counts) {
    if (!e || !v) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (const char *why = view_error(*v)) {
        e->err = why;
        return BH_E_INVALID;
    }
    const size_t npix = (size_t)v->width * (size_t)v->height;
    const int64_t n = e->trc_n;
    if (n <= 0) {  // nothing drawn: no device work
        if (owner) std::memset(owner, 0xFF, sizeof(uint32_t) * npix);
        if (counts) std::memset(counts, 0, sizeof(uint32_t) * npix);
        return BH_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    // bh_render_bodies' working planes and kernels; the list's own order stands for cidx and
    // there is no mass plane (no colour); its kernel timing is left as it was
    const size_t pad = render_padded_pixels(v->width, v->height);
    TRY(render_buffers(e, pad, false, owner != nullptr, counts != nullptr));
    e->rnd_clean = false;
    render_raster(n, e->trc, e->trc + (size_t)n, nullptr, nullptr, *v, e->rnd_packed,
                  counts ? e->rnd_cnt : nullptr, e->stream);
    HIPCHK(e, hipGetLastError());
    render_resolve(pad, e->rnd_packed, counts ? e->rnd_cnt : nullptr, nullptr,
                   owner ? e->rnd_owner : nullptr, counts ? e->rnd_counts : nullptr, e->stream);
    HIPCHK(e, hipGetLastError());
    e->rnd_clean = true;
    if (owner)
        HIPCHK(e, hipMemcpyAsync(owner, e->rnd_owner, sizeof(uint32_t) * npix,
                                 hipMemcpyDeviceToHost, e->stream));
    if (counts)
        HIPCHK(e, hipMemcpyAsync(counts, e->rnd_counts, sizeof(uint32_t) * npix,
                                 hipMemcpyDeviceToHost, e->stream));
    SYNC(e, e->stream);
    return BH_OK;
}

int bh_get_quads(bh_engine *e, double *cx, double *cy, double *h, int64_t cap, int64_t *n_out) {
    if (!e || cap < 0 || (cap > 0 && (!cx || !cy || !h))) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (e->multi) {  // every member builds getTreeForDebug's tree (the same jitter in every
                     // replica); member 0 walks it
        const int rc = multi_fan(e, [](bh_engine *m, int) {
            TRY(comm_refused(m));
            return fail_multi_rank(m, quads_prepare(m));
        }, false);
        if (rc != BH_OK) return rc;
        const int rc0 = bh_get_quads(MULTI_M0(e), cx, cy, h, cap, n_out);
        if (rc0 != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc0;
    }
    COMM_GUARD(e);
    TRY(fail_multi_rank(e, quads_prepare(e)));
    const int64_t n = e->n;
    std::vector<uint64_t> keys((size_t)n);
    std::vector<int8_t> cpl((size_t)n);
    std::vector<uint32_t> base((size_t)n + 1);
    SYNC(e, e->stream);
    // lastTree kept aside by a pipelined last step, or the tree in the build buffers
    const bool aside = e->tree_valid && e->lt_aside;
    if (n > 0) {
        HIPCHK(e, hipMemcpy(keys.data(), aside ? e->lt_keys : e->keys_s, sizeof(uint64_t) * n,
                            hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(cpl.data(), aside ? e->lt_cpl : e->cpl, n, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(base.data(), aside ? e->lt_base : e->base, sizeof(uint32_t) * (n + 1),
                            hipMemcpyDeviceToHost));
    }
    int64_t M = 0;
    const uint64_t SENT = sentinel_key(e->geo.J);
    while (M < n && keys[(size_t)M] != SENT) ++M;
    QuadWalker w{e->geo, keys, cpl, base, aside ? e->nodes_alt : e->nodes, cx, cy, h, cap};
    w.rec(0, 0, M, e->geo.root_cx, e->geo.root_cy, e->geo.root_h);
    if (w.rc != BH_OK) return w.rc;
    if (n_out) *n_out = w.k;
    return w.k > cap ? BH_E_CAPACITY : BH_OK;
}

// The overlay's working planes (zero between calls), the staged count plane and the events.
static int quads_buffers(bh_engine *e, size_t npix, bool image, bool direct) {
    if (image && npix != e->qd_pix) {  // another view size: made anew
        uint32_t **all[] = {&e->qd_rowd, &e->qd_cold, &e->qd_dir, &e->qd_out};
        for (uint32_t **q : all) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        e->qd_pix = npix;
    }
    if (image) {
        uint32_t **work[] = {&e->qd_rowd, &e->qd_cold, direct ? &e->qd_dir : nullptr};
        for (uint32_t **q : work) {
            if (!q || *q) continue;
            TRY(dev_alloc(e, *q, npix));
            HIPCHK(e, hipMemsetAsync(*q, 0, sizeof(uint32_t) * npix, e->stream));
        }
        if (!e->qd_out) TRY(dev_alloc(e, e->qd_out, npix));
        if (!e->qd_clean) {  // a call that failed between its kernels left the planes as they were
            for (uint32_t *q : {e->qd_rowd, e->qd_cold, e->qd_dir})
                if (q) HIPCHK(e, hipMemsetAsync(q, 0, sizeof(uint32_t) * npix, e->stream));
            e->qd_clean = true;
        }
    }
    if (!e->qd_count) TRY(dev_alloc(e, e->qd_count, (size_t)QUADS_COUNT_WORDS));
    return BH_OK;
}

// The tree bh_get_quads walks (after the same quads_prepare), rasterised on the device.
static int render_quads_state(bh_engine *e, const bh_view &v, uint32_t *lines, int64_t *n_quads) {
    const size_t npix = (size_t)v.width * (size_t)v.height;
    // BH_QUADS_DIRECT=0: one-pixel cells through the difference planes too (A/B; the same bytes).
    // Read per call, so that one process can interleave the two (tools/quads_bench.py).
    const char *env = std::getenv("BH_QUADS_DIRECT");
    const bool direct = env ? std::atoi(env) != 0 : true;
    // BH_QUADS_COMBINE=0: every one-pixel cell issues its own atomic (A/B; the same bytes)
    env = std::getenv("BH_QUADS_COMBINE");
    const bool combine = env ? std::atoi(env) != 0 : true;
    TRY(quads_buffers(e, npix, lines != nullptr, direct));
    // lastTree kept aside by a pipelined last step, or the tree in the build buffers
    const bool aside = e->tree_valid && e->lt_aside;
    const QuadTree t{aside ? e->lt_keys : e->keys_s, aside ? e->lt_cpl : e->cpl,
                     aside ? e->lt_base : e->base, aside ? e->nodes_alt : e->nodes, e->n};
    unsigned long long part[QUADS_COUNT_WORDS];
    HIPCHK(e, hipMemsetAsync(e->qd_count, 0, sizeof(part), e->stream));
    if (lines) e->qd_clean = false;
    TRY(e->qd_sw.start(e, e->stream));
    quads_render(t, e->geo, v, e->qd_rowd, e->qd_cold, direct ? e->qd_dir : nullptr, combine,
                 lines ? e->qd_out : nullptr, e->qd_count, e->stream);
    HIPCHK(e, hipGetLastError());
    TRY(e->qd_sw.stop(e, e->stream));
    if (lines) e->qd_clean = true;
    if (lines)
        HIPCHK(e, hipMemcpyAsync(lines, e->qd_out, sizeof(uint32_t) * npix, hipMemcpyDeviceToHost,
                                 e->stream));
    HIPCHK(e, hipMemcpyAsync(part, e->qd_count, sizeof(part), hipMemcpyDeviceToHost, e->stream));
    SYNC(e, e->stream);
    unsigned long long cells = 0;
    for (int k = 0; k < QUADS_COUNT_STRIPES; ++k) cells += part[k * QUADS_COUNT_STRIDE];
    if (n_quads) *n_quads = (int64_t)cells;
    return BH_OK;
}

int bh_render_quads(bh_engine *e, const bh_view *v, uint32_t *lines, int64_t *n_quads) {
    if (!e || !v) return BH_E_INVALID;
    ASYNC_GUARD(e);
    if (const char *why = view_error(*v)) {
        e->err = why;
        return BH_E_INVALID;
    }
    if (e->multi) {  // as bh_get_quads: every member prepares the tree, member 0 answers
        const int rc = multi_fan(e, [](bh_engine *m, int) {
            TRY(comm_refused(m));
            return fail_multi_rank(m, quads_prepare(m));
        }, false);
        if (rc != BH_OK) return rc;
        const int rc0 = bh_render_quads(MULTI_M0(e), v, lines, n_quads);
        if (rc0 != BH_OK) e->err = bh_last_error(MULTI_M0(e));
        return rc0;
    }
    COMM_GUARD(e);
    TRY(fail_multi_rank(e, quads_prepare(e)));
    return render_quads_state(e, *v, lines, n_quads);
}

int bh_render_quads_kernel_ms(const bh_engine *e, double *ms) {
    return kernel_ms(e, &bh_engine::qd_sw, ms);
}

int bh_last_removed(const bh_engine *e, int64_t *idx, int64_t cap, int64_t *n_out) {
    if (!e || cap < 0 || (cap > 0 && !idx)) return BH_E_INVALID;
    // (a call begun by bh_step_begin writes the log: read it after bh_step_end)
    if (e->async_running && std::this_thread::get_id() != e->step_thr.get_id()) return BH_E_STATE;
    return last_removed(e, idx, cap, n_out);
}

static int last_removed(const bh_engine *e, int64_t *idx, int64_t cap, int64_t *n_out) {
    e = MULTI_M0(e);
    // caller indices are not renumbered inside a call, so the log is already relative to the
    // list before the call
    if (n_out) *n_out = (int64_t)e->removed.size();
    if ((int64_t)e->removed.size() > cap) return BH_E_CAPACITY;
    for (size_t i = 0; i < e->removed.size(); ++i) idx[i] = e->removed[i];
    return BH_OK;
}

int bh_last_timings(const bh_engine *e, double *out5) {
    if (!e || !out5) return BH_E_INVALID;
    e = MULTI_M0(e);
    for (int k = 0; k < kPhases; ++k) out5[k] = e->phase_ms[k];
    return BH_OK;
}

int64_t bh_last_tree_nodes(const bh_engine *e) {
    if (e) e = MULTI_M0(e);
    if (!e || e->n <= 0) return 0;
    uint32_t T = 0;
    const uint32_t *base = e->lt_aside ? e->lt_base : e->base;
    if (hipMemcpy(&T, base + e->n, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return T;
}

int bh_traverse_kernel_ms(const bh_engine *e, double *avg_ms, int64_t *launches) {
    if (!e || !avg_ms) return BH_E_INVALID;
    e = MULTI_M0(e);
    *avg_ms = e->trav_launches ? e->trav_ms_sum / (double)e->trav_launches : 0.0;
    if (launches) *launches = e->trav_launches;
    return BH_OK;
}

int bh_traverse_kernel_samples(const bh_engine *e, double *ms, int64_t cap, int64_t *n_out) {
    if (!e || cap < 0 || (cap > 0 && !ms)) return BH_E_INVALID;
    e = MULTI_M0(e);
    const int64_t n = (int64_t)e->trav_samples.size();
    if (n_out) *n_out = n;
    if (n > cap) return BH_E_CAPACITY;
    for (int64_t i = 0; i < n; ++i) ms[i] = e->trav_samples[(size_t)i];
    return BH_OK;
}

int bh_traversal_stats(const bh_engine *e, int64_t *lane_visits, int64_t *wave_iters,
                       int64_t *waves) {
    if (!e || !lane_visits || !wave_iters || !waves) return BH_E_INVALID;
    e = MULTI_M0(e);
    *lane_visits = e->stat_lane_visits;
    *wave_iters = e->stat_wave_iters;
    *waves = e->stat_waves;
    return BH_OK;
}

int bh_traversal_counters(const bh_engine *e, int64_t *out5) {
    if (!e || !out5) return BH_E_INVALID;
    e = MULTI_M0(e);
    out5[0] = e->stat_lane_visits;
    out5[1] = e->stat_lane_contrib;
    out5[2] = e->stat_wave_iters;
    out5[3] = e->stat_wave_blocks;
    out5[4] = e->stat_waves;
    return BH_OK;
}

int bh_let_stats(const bh_engine *e, int64_t *out4) {
    if (!e || !out4) return BH_E_INVALID;
    e = MULTI_M0(e);
    out4[4] = e->let_overflows;
    out4[0] = e->let_builds;
    out4[1] = e->full_builds;
    out4[2] = e->let_last_sub;
    uint32_t T = 0;
    if (e->L.posc &&
        hipMemcpy(&T, e->L.posc + LET_CELLS, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return BH_E_DEVICE;
    out4[3] = T;
    return BH_OK;
}

int bh_set_profiling(bh_engine *e, int enabled) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    MULTI_BOTH(e, bh_set_profiling(m_, enabled));
    e->profiling = enabled != 0;
    return BH_OK;
}

int bh_shard_range(int64_t n, int rank, int world, int round, int64_t *lo, int64_t *hi) {
    if (n < 0 || world < 1 || rank < 0 || rank >= world || round < 0 ||
        round >= BH_SHARD_ROUNDS || !lo || !hi)
        return BH_E_INVALID;
    const GatherLayout L = shard_layout(n, world);  // whole wavefronts
    *lo = std::min<int64_t>(n, (int64_t)rank * L.span + L.off[round]);  // in the own range
    *hi = std::min<int64_t>(n, (int64_t)rank * L.span + L.off[round + 1]);
    return BH_OK;
}

int64_t bh_gather_slot(int64_t n, int world, int64_t lane) {
    if (n < 0 || world < 1 || lane < 0) return -1;
    return gather_slot(shard_layout(n, world), lane);
}

// Every value comes from the function the build or the traversal itself branches on.
int bh_launch_plan(const bh_params *p, int64_t n, int64_t *out, int64_t cap, int64_t *n_out) {
    if (!p || n < 0 || !n_out || cap < 0 || (cap > 0 && !out)) return BH_E_INVALID;
    *n_out = BH_PLAN_FIELDS;
    Geometry g;
    std::string err;
    if (make_geometry(*p, g, err) != BH_OK) return BH_E_INVALID;
    int64_t f[BH_PLAN_FIELDS] = {};
    if (n > 0) {
        uint32_t P = 0;
        f[BH_PLAN_SMALL_FRONT] = small_front_for(n, P) ? 1 : 0;
        f[BH_PLAN_SMALL_FRONT_P] = f[BH_PLAN_SMALL_FRONT] ? (int64_t)P : 0;
        f[BH_PLAN_CELL_DEPTH] = cell_table_depth(g.J, n);
        f[BH_PLAN_SORT_BUCKETS] = sort_buckets(n);
        f[BH_PLAN_COM_CHUNKS] = com_chunks(n);
        f[BH_PLAN_SPAN_GROUPS] = span_groups(span_stride_for(n));  // (capacity = n)
        // (the scratch of any engine holds at least the block sums: tree_scratch_bytes)
        f[BH_PLAN_OWN_SCAN] = own_base_scan(n, base_scan_sums_bytes(n)) ? 1 : 0;
        const size_t ncap = node_capacity(n, g.J);
        const bool ordered = wave_order_used(n);
        const TraverseShape t1 = traverse_shape(ncap, 0, n, KICK_DRIFT, false, ordered);
        const TraverseShape t2 = traverse_shape(ncap, 0, n, KICK_ONLY, false, ordered);
        f[BH_PLAN_BFS] = t1.bfs ? 1 : 0;
        f[BH_PLAN_BFS_BITS] = 32 * (int64_t)t1.bm_words;
        f[BH_PLAN_BPW] = t1.bpw;
        f[BH_PLAN_WPB] = t1.wpb;
        f[BH_PLAN_XCD_GROUPS] = t1.xcd_full;
        f[BH_PLAN_KICK_BPW] = t2.bpw;
        f[BH_PLAN_KICK_WPB] = t2.wpb;
        f[BH_PLAN_KICK_XCD_GROUPS] = t2.xcd_full;
        f[BH_PLAN_ORDER_RUNS] = (int64_t)wave_order_runs(n);
        f[BH_PLAN_NODE_ADDR64] = node_off32(ncap) ? 0 : 1;
    }
    for (int64_t i = 0; i < cap && i < BH_PLAN_FIELDS; ++i) out[i] = f[i];
    return BH_OK;
}

int bh_selftest_fast_math(int device, int64_t n, uint64_t seed, int64_t *mismatches) {
    if (!mismatches || n < 0) return BH_E_INVALID;
    *mismatches = -1;
    unsigned long long *d_bad = nullptr, h_bad = 0;
    if (hipSetDevice(device) != hipSuccess) return BH_E_DEVICE;
    if (hipMalloc((void **)&d_bad, sizeof(*d_bad)) != hipSuccess) return BH_E_DEVICE;
    bool ok = hipMemset(d_bad, 0, sizeof(*d_bad)) == hipSuccess &&
              bh::selftest_fast_math(n, seed, d_bad, nullptr) == hipSuccess &&
              hipMemcpy(&h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_bad);
    if (!ok) return BH_E_DEVICE;
    *mismatches = (int64_t)h_bad;
    return BH_OK;
}

int bh_synchronize(bh_engine *e) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    MULTI_ALL(e, bh_synchronize(m_));
    HIPCHK(e, hipSetDevice(e->device));
    SYNC(e, e->stream);
    return BH_OK;
}

int bh_comm_ranks(const bh_engine *e, int32_t *nranks, int32_t *rank) {
    if (!e || !nranks || !rank) return BH_E_INVALID;
    e = MULTI_M0(e);
    *nranks = 0;
    *rank = e->rank;
    if (!e->comm) return BH_OK;
    int c = 0, r = 0;
    if (ncclCommCount(e->comm, &c) != ncclSuccess || ncclCommUserRank(e->comm, &r) != ncclSuccess)
        return BH_E_COMM;
    *nranks = c;
    *rank = r;
    return BH_OK;
}

int bh_debug_inject(bh_engine *e, int what) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    MULTI_ALL(e, bh_debug_inject(m_, what));  // (one member alone: bh_multi_member)
    if (what < 1 || what >= 300) {
        e->err = "bh_debug_inject: unknown fault";
        return BH_E_INVALID;
    }
    if (what == 99) {  // the carried tree (the next call's first) raises its error flag now
        if (!e->carried_flags || !e->prebuilt) {
            e->err = "bh_debug_inject(99): no tree carried to the next call";
            return BH_E_STATE;
        }
        HIPCHK(e, hipMemsetAsync(e->scalars + 10, 1, sizeof(uint32_t), e->stream));
        return BH_OK;
    }
    if (what == 1) e->inject_guard = true;
    else if (what >= 200) e->inject_barrier = what - 200;
    else if (what >= 100) e->inject_coll = what - 100;
    else e->inject_build = what - 2;
    return BH_OK;
}

int bh_progress(const bh_engine *e, int64_t *out4) {
    if (!e || !out4) return BH_E_INVALID;
    e = MULTI_M0(e);  // (a member's own: bh_multi_member)
    out4[0] = e->prog_api.load();
    out4[1] = e->prog_coll.load();
    out4[2] = e->prog_site.load();
    const bool failed = e->comm_failed || (multi_rank(e) && peers_aborted(e));  // (will refuse)
    out4[3] = (e->prog_busy.load() ? 1 : 0) | (failed ? 2 : 0) | (e->comm_lost ? 4 : 0);
    return BH_OK;
}

int bh_multi_world(const bh_engine *e) {
    if (!e) return 0;
    return e->multi && !e->use_one ? multi_world(e->multi) : 1;
}

bh_engine *bh_multi_member(bh_engine *e, int rank) {
    if (!e) return nullptr;
    if (!e->multi) return rank == 0 ? e : nullptr;
    if (e->use_one) return rank == 0 ? e->one : nullptr;
    return multi_member(e->multi, rank);
}

int bh_collective_log(const bh_engine *e, int64_t *out4, int64_t cap, int64_t *n_out) {
    if (!e || cap < 0 || (cap > 0 && !out4)) return BH_E_INVALID;
    e = MULTI_M0(e);
    const int64_t n = (int64_t)e->coll_log.size() / 4;
    if (n_out) *n_out = n;
    if (n > cap) return BH_E_CAPACITY;
    std::copy(e->coll_log.begin(), e->coll_log.end(), out4);
    return BH_OK;
}

int bh_collective_log_clear(bh_engine *e) {
    if (!e) return BH_E_INVALID;
    ASYNC_GUARD(e);
    MULTI_BOTH(e, bh_collective_log_clear(m_));
    e->coll_log.clear();
    return BH_OK;
}

}  // extern "C"
