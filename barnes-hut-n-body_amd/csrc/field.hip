// Field query over the flattened quadtree: acceleration and potential at probe points that are
// not bodies of the system (bh_compute_field, include/bh_engine.h), and the same on a regular grid
// whose points the kernel forms itself (bh_compute_field_grid: k_field_grid and its reductions,
// after k_field_keys), and the same walk carried through time for bh_step's tracers
// (k_tracer_step: the leapfrog's kick and drift as the walk's epilogue).
//
// Probe j is a Body(px, py, 0, 0, pm) that is NOT in the tree.  BHTree.accumulateForce for such a
// body (BHA:215-239) skips massless nodes (BHA:216), never meets "its own leaf" -- the identity
// test of BHA:219 cannot match -- so it takes EVERY non-empty leaf, and takes an internal node iff
// s2 < theta2 * dist2 (BHA:226-228), else visits its children in order.  Every taken node adds,
// in that pre-order,
//     dx = comX - px;  dy = comY - py;  r2 = dx*dx + dy*dy + soft2
//     invR = 1.0 / sqrt(r2);  invR2 = 1.0 / r2;  f = (G * pm) * m * invR2          (BHA:250-259)
//     fx += f * dx * invR;  fy += f * dy * invR;  s += m * invR                     (from +0.0)
// and a = F / pm (BHA:390-391), phi = -(G * s) (the term of bh_compute_potential).  This is what
// the engine already computes for a body outside the root cell (BHA:126: not inserted, walked).
//
// The walk is the probe walk of cursor_walk.hpp (probe_walk, shared with potential.hip) for a lane
// without a slot: one lane = one probe, one wave-shared pre-order cursor, every lane's own
// criterion by ballot.  It is not the force walk because a probe has no slot: walk<false> skips
// the leaf whose body slot equals the lane's slot and k_potential compares every leaf against it,
// while probe i must feel the body in slot i; and the fast force walk relies on the own leaf's
// term being +-0, while a probe that sits on a body owes that body's full potential term
// m / sqrt(soft2).  So no path here compares a leaf with anything, and no term is ever excused.
// One point-force block serves both results: the potential's term reuses the block's invR (one
// multiply and one add more; never fused: the build contracts nothing).
#include <rocprim/device/device_radix_sort.hpp>

#include "bh_device.hpp"
#include "cursor_walk.hpp"

namespace bh {
namespace {

constexpr int KEY_TB = 256;

// What the three walking kernels do between a lane's point and its sums: the guards of the fast
// path over the wave's valid lanes, then the fast or the exact probe walk.  d_T null: no tree was
// built (no bodies).  The sums start at +0.0; an invalid lane never becomes active.
template <bool OFF32, int SUMS>
__device__ __forceinline__ void probe_eval(const Node *__restrict__ nodes,
                                           const uint32_t *__restrict__ d_T,
                                           const ForceParams &fp, double s2root, double bx,
                                           double by, double bm, bool valid, double &fx,
                                           double &fy, double &s) {
    const double Gm = fp.G * bm;  // (Config.G * b.m) is evaluated first (BHA:256)
    const double soft2 = fp.soft2, theta2 = fp.theta2;
    const uint32_t resume = valid ? 0u : 0xFFFFFFFFu;  // active at `cur` iff cur >= resume
    const uint32_t T = d_T ? __builtin_amdgcn_readfirstlane(*d_T) : 0u;
    const bool lane_ok = lane_fast_ok(bx, by, soft2) &&
                         __builtin_fabs(Gm) <= 1.7976931348623157e308;  // (false for a NaN)
    const bool fast = fast_s2_ok(s2root) && __ballot(valid && !lane_ok) == 0ull;
    fx = fy = s = 0.0;
    if (fast)
        probe_walk<true, OFF32, false, SUMS>(nodes, T, bx, by, Gm, soft2, theta2, s2root, 0u,
                                             resume, fx, fy, s);
    else
        probe_walk<false, OFF32, false, SUMS>(nodes, T, bx, by, Gm, soft2, theta2, s2root, 0u,
                                              resume, fx, fy, s);
}

// Wave v walks the bpw lanes [bpw v, bpw v + bpw); lane q holds probe order[q] and writes its
// results straight to that caller index.  d_T null: no tree was built (no bodies).
template <bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_field(const Node *__restrict__ nodes,
                                                        const uint32_t *__restrict__ d_T,
                                                        const double *__restrict__ px,
                                                        const double *__restrict__ py,
                                                        const double *__restrict__ pm,
                                                        const uint32_t *__restrict__ order,
                                                        int64_t n, ForceParams fp, double s2root,
                                                        double *__restrict__ ax,
                                                        double *__restrict__ ay,
                                                        double *__restrict__ phi, uint32_t bpw,
                                                        uint32_t wpb) {
    const uint32_t v = xcd_run_wave(wpb);
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t q = (int64_t)v * bpw + lane;
    const bool valid = lane < bpw && q < n;
    const int64_t j = valid ? (int64_t)order[q] : 0;  // the probe's caller index
    const double bx = valid ? px[j] : 0.0;
    const double by = valid ? py[j] : 0.0;
    const double bm = valid && pm ? pm[j] : 1.0;
    double fx, fy, s;
    probe_eval<OFF32, PROBE_BOTH>(nodes, d_T, fp, s2root, bx, by, bm, valid, fx, fy, s);
    if (!valid) return;
    ax[j] = fx / bm;  // BHA:390-391
    ay[j] = fy / bm;
    phi[j] = -(fp.G * s);
}

// bh_step's tracers (bh_set_tracers): tracer t is a probe of mass 1.0 that is carried through
// time.  Guards, walk and result arithmetic are k_field's for pm = NULL (G * 1.0 and fx / 1.0 are
// exact); instead of storing a and phi the lane applies the leapfrog's lines to its own tracer in
// registers -- KICK_DRIFT = BHA:414-422, KICK_ONLY = BHA:429-432, the operations of k_kick_drift /
// k_kick in their order, never fused -- and writes the tracer's values back in place, by list
// index.  The potential's sum is not used here, so the walk is asked for the force alone.
template <int KICK, bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_tracer_step(const Node *__restrict__ nodes,
                                                              const uint32_t *__restrict__ d_T,
                                                              double *__restrict__ tx,
                                                              double *__restrict__ ty,
                                                              double *__restrict__ tvx,
                                                              double *__restrict__ tvy,
                                                              const uint32_t *__restrict__ order,
                                                              int64_t n, ForceParams fp,
                                                              double s2root, double dtHalf,
                                                              double dt, uint32_t bpw,
                                                              uint32_t wpb) {
    static_assert(KICK == KICK_DRIFT || KICK == KICK_ONLY, "a tracer walk always kicks");
    const uint32_t v = xcd_run_wave(wpb);
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t q = (int64_t)v * bpw + lane;
    const bool valid = lane < bpw && q < n;
    const int64_t j = valid ? (int64_t)order[q] : 0;  // the tracer's list index
    const double bx = valid ? tx[j] : 0.0;
    const double by = valid ? ty[j] : 0.0;
    double fx, fy, s;
    probe_eval<OFF32, PROBE_FORCE>(nodes, d_T, fp, s2root, bx, by, 1.0, valid, fx, fy, s);
    if (!valid) return;
    const double ax = fx / 1.0;  // BHA:390-391
    const double ay = fy / 1.0;
    const double vx = tvx[j] + ax * dtHalf;  // BHA:414-415 / BHA:429-430
    const double vy = tvy[j] + ay * dtHalf;
    tvx[j] = vx;
    tvy[j] = vy;
    if (KICK == KICK_DRIFT) {  // BHA:416-417
        tx[j] = bx + vx * dt;
        ty[j] = by + vy * dt;
    }
}

// The build's own key of a probe's position (total: a NaN or out-of-root probe takes the
// sentinel), its 32-bit prefix as the build sorts it, and the probe's index.
__global__ __launch_bounds__(KEY_TB) void k_field_keys(int64_t n, const double *__restrict__ px,
                                                       const double *__restrict__ py, Geometry g,
                                                       uint32_t *__restrict__ key,
                                                       uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * KEY_TB + threadIdx.x;
    if (i >= n) return;
    key[i] = (uint32_t)(morton_key(g, px[i], py[i], false) >> key32_shift(g.J));
    idx[i] = (uint32_t)i;
}

// bh_compute_field_grid: wave v is tile zorder_tile(v) of the grid, lane l its point (l % tile_w,
// l / tile_w) -- a compact patch of the plane, so the lanes of a wave, the waves of a workgroup
// and the waves of an XCD run open the same cells.  The coordinates are formed here from the six
// grid values (one multiply, one add; the build contracts nothing); the guards, the walk and the
// result arithmetic are k_field's for pm = NULL (G * 1.0 and fx / 1.0 are exact).  Lanes past the
// right or bottom edge are invalid as k_field's are; each valid lane stores straight to the
// row-major planes (an 8 x 8 tile: eight 64-byte row segments per plane), a null plane is not
// stored.
template <bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_field_grid(const Node *__restrict__ nodes,
                                                             const uint32_t *__restrict__ d_T,
                                                             bh_field_grid g, ForceParams fp,
                                                             double s2root,
                                                             double *__restrict__ ax,
                                                             double *__restrict__ ay,
                                                             double *__restrict__ phi,
                                                             FieldGridShape sh) {
    const uint32_t v = __builtin_amdgcn_readfirstlane(xcd_run_wave(sh.wpb));
    if (v >= sh.tiles) return;  // (the last workgroup's spare waves)
    uint32_t tx, ty;
    zorder_tile(v, sh.tiles_x, sh.tiles_y, tx, ty);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lx = lane & (sh.tile_w - 1u), ly = lane >> __builtin_ctz(sh.tile_w);
    const uint32_t c = tx * sh.tile_w + lx, r = ty * sh.tile_h + ly;
    const bool valid = ly < sh.tile_h && c < (uint32_t)g.nx && r < (uint32_t)g.ny;
    const double bx = valid ? g.x0 + (double)c * g.dx : 0.0;
    const double by = valid ? g.y0 + (double)r * g.dy : 0.0;
    double fx, fy, s;
    probe_eval<OFF32, PROBE_BOTH>(nodes, d_T, fp, s2root, bx, by, 1.0, valid, fx, fy, s);
    if (!valid) return;
    const int64_t j = (int64_t)r * g.nx + c;
    if (ax) ax[j] = fx / 1.0;  // BHA:390-391
    if (ay) ay[j] = fy / 1.0;
    if (phi) phi[j] = -(fp.G * s);
}

// bh_field_grid_stats: the neutral element and the merge of two summaries of disjoint index sets.
// Minimum and maximum under (value, index) -- zeros equal by value, the lower index first -- are
// associative and commutative, so the result does not depend on how the indices were grouped.
constexpr int GST_TB = 256;
constexpr int GST_MAX_BLOCKS = 1024;

__device__ __forceinline__ bh_field_grid_stats gstat_none() {
    return bh_field_grid_stats{0, -1, 0.0, 0.0, 0, -1, 0.0};
}
__device__ __forceinline__ void gstat_merge(bh_field_grid_stats &a, const bh_field_grid_stats &b) {
    if (b.n_phi > 0) {
        if (a.n_phi == 0 || b.phi_min < a.phi_min ||
            (b.phi_min == a.phi_min && b.i_phi_min < a.i_phi_min)) {
            a.phi_min = b.phi_min;
            a.i_phi_min = b.i_phi_min;
        }
        if (a.n_phi == 0 || b.phi_max > a.phi_max) a.phi_max = b.phi_max;
        a.n_phi += b.n_phi;
    }
    if (b.n_acc > 0) {
        if (a.n_acc == 0 || b.a2_max > a.a2_max ||
            (b.a2_max == a.a2_max && b.i_a2_max < a.i_a2_max)) {
            a.a2_max = b.a2_max;
            a.i_a2_max = b.i_a2_max;
        }
        a.n_acc += b.n_acc;
    }
}
__device__ __forceinline__ void gstat_block(bh_field_grid_stats &v, bh_field_grid_stats *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int w = GST_TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) gstat_merge(lds[threadIdx.x], lds[threadIdx.x + w]);
        __syncthreads();
    }
}

// workgroup b summarises the row-major indices [b chunk, b chunk + chunk)
__global__ __launch_bounds__(GST_TB) void k_grid_stats_partial(int64_t n, int64_t chunk,
                                                               const double *__restrict__ ax,
                                                               const double *__restrict__ ay,
                                                               const double *__restrict__ phi,
                                                               bh_field_grid_stats *__restrict__ part) {
    __shared__ bh_field_grid_stats lds[GST_TB];
    bh_field_grid_stats v = gstat_none();
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += GST_TB) {
        bh_field_grid_stats one = gstat_none();
        const double p = phi[i], x = ax[i], y = ay[i];
        if (__builtin_isfinite(p)) {
            one.n_phi = 1;
            one.i_phi_min = i;
            one.phi_min = one.phi_max = p;
        }
        if (__builtin_isfinite(x) && __builtin_isfinite(y)) {
            one.n_acc = 1;
            one.i_a2_max = i;
            one.a2_max = x * x + y * y;
        }
        gstat_merge(v, one);
    }
    gstat_block(v, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = lds[0];
}

__global__ __launch_bounds__(GST_TB) void k_grid_stats_final(int blocks,
                                                             const bh_field_grid_stats *__restrict__ part,
                                                             bh_field_grid_stats *__restrict__ out) {
    __shared__ bh_field_grid_stats lds[GST_TB];
    bh_field_grid_stats v = gstat_none();
    for (int q = threadIdx.x; q < blocks; q += GST_TB) gstat_merge(v, part[q]);
    gstat_block(v, lds);
    if (threadIdx.x == 0) *out = lds[0];
}

}  // namespace

FieldGridShape field_grid_shape(int32_t nx, int32_t ny) {
    const uint32_t bpw = bodies_per_wave((int64_t)nx * ny);
    FieldGridShape sh;
    sh.tile_w = sh.tile_h = 8;
    for (uint32_t q = TB; q > bpw; q >>= 1) {  // rows first: 8 x 4, 4 x 4, 4 x 2, ...
        if (sh.tile_h == sh.tile_w)
            sh.tile_h >>= 1;
        else
            sh.tile_w >>= 1;
    }
    sh.tiles_x = ((uint32_t)nx + sh.tile_w - 1) / sh.tile_w;
    sh.tiles_y = ((uint32_t)ny + sh.tile_h - 1) / sh.tile_h;
    sh.tiles = sh.tiles_x * sh.tiles_y;
    sh.wpb = waves_per_group(sh.tiles, bpw);
    return sh;
}

void field_grid_walk(const Node *nodes, size_t node_cap, const uint32_t *d_T,
                     const bh_field_grid &g, const Geometry &geo, const ForceParams &fp, double *ax,
                     double *ay, double *phi, hipStream_t s) {
    const FieldGridShape sh = field_grid_shape(g.nx, g.ny);
    const unsigned grid = (sh.tiles + sh.wpb - 1) / sh.wpb;
    if (node_off32(node_cap))
        k_field_grid<true><<<grid, TB * sh.wpb, 0, s>>>(nodes, d_T, g, fp, geo.s2[0], ax, ay, phi,
                                                        sh);
    else
        k_field_grid<false><<<grid, TB * sh.wpb, 0, s>>>(nodes, d_T, g, fp, geo.s2[0], ax, ay, phi,
                                                         sh);
}

size_t field_grid_stat_partials() { return (size_t)GST_MAX_BLOCKS + 1; }

void field_grid_stats(int64_t n, const double *ax, const double *ay, const double *phi,
                      bh_field_grid_stats *part, bh_field_grid_stats *out, hipStream_t s) {
    // whole workgroup strides per chunk, at most GST_MAX_BLOCKS chunks
    int64_t chunk = (n + GST_MAX_BLOCKS - 1) / GST_MAX_BLOCKS;
    chunk = (chunk + GST_TB - 1) / GST_TB * GST_TB;
    if (chunk < GST_TB) chunk = GST_TB;
    const int blocks = n > 0 ? (int)((n + chunk - 1) / chunk) : 1;
    k_grid_stats_partial<<<blocks, GST_TB, 0, s>>>(n, chunk, ax, ay, phi, part);
    k_grid_stats_final<<<1, GST_TB, 0, s>>>(blocks, part, out);
}

size_t field_sort_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 32u);
    return bytes;
}

hipError_t field_order(int64_t n, const double *px, const double *py, const Geometry &g,
                       uint32_t *key, uint32_t *key_s, uint32_t *idx, uint32_t *order,
                       void *scratch, size_t scratch_bytes, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    k_field_keys<<<(unsigned)((n + KEY_TB - 1) / KEY_TB), KEY_TB, 0, s>>>(n, px, py, g, key, idx);
    hipError_t st = hipGetLastError();
    if (st != hipSuccess) return st;
    size_t bytes = scratch_bytes;
    return rocprim::radix_sort_pairs(scratch, bytes, key, key_s, idx, order, (size_t)n, 0u, 32u,
                                     s);
}

void field_walk(const Node *nodes, size_t node_cap, const uint32_t *d_T, const double *px,
                const double *py, const double *pm, const uint32_t *order, int64_t n,
                const Geometry &g, const ForceParams &fp, double *ax, double *ay, double *phi,
                hipStream_t s) {
    if (n <= 0) return;
    const WalkShape w = walk_shape(n);
    if (node_off32(node_cap))
        k_field<true><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, px, py, pm, order, n, fp, g.s2[0],
                                                    ax, ay, phi, w.bpw, w.wpb);
    else
        k_field<false><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, px, py, pm, order, n, fp, g.s2[0],
                                                     ax, ay, phi, w.bpw, w.wpb);
}

#ifndef BH_TRACER_REORDER
// steps between re-orderings of the tracers' lane map.  C3 with 10^6 tracers on the bodies' start
// positions, ms per step over 128-step calls, two alternating rounds (DESIGN.md §15,
// profiles/tracers_timing.jsonl): R = 1 4.08 / 4.08, 4 4.44 / 4.44, 16 5.43 / 5.47, 64 6.60 /
// 6.69 against 1.48 without tracers -- the keys and the radix sort of 10^6 tracers cost less
// than one step's loss of lane coherence
#define BH_TRACER_REORDER 1
#endif
static_assert(BH_TRACER_REORDER >= 1, "the lane map is re-made every R >= 1 steps");

TracerShape tracer_shape(int64_t n) {
    const WalkShape w = walk_shape(n);
    TracerShape sh;
    sh.bpw = w.bpw;
    sh.waves = w.waves;
    sh.wpb = w.wpb;
    sh.reorder = BH_TRACER_REORDER;
    return sh;
}

void tracer_step(const Node *nodes, size_t node_cap, const uint32_t *d_T, double *tx, double *ty,
                 double *tvx, double *tvy, const uint32_t *order, int64_t n, const Geometry &g,
                 const ForceParams &fp, KickMode kick, double dtHalf, double dt, hipStream_t s) {
    if (n <= 0) return;
    const bool off32 = node_off32(node_cap);
    const TracerShape sh = tracer_shape(n);
    const unsigned grid = (sh.waves + sh.wpb - 1) / sh.wpb, tb = TB * sh.wpb;
#define BH_TRACER_LAUNCH(K, O)                                                                    \
    k_tracer_step<K, O><<<grid, tb, 0, s>>>(nodes, d_T, tx, ty, tvx, tvy, order, n, fp, g.s2[0], \
                                            dtHalf, dt, sh.bpw, sh.wpb)
    if (kick == KICK_DRIFT) {
        if (off32)
            BH_TRACER_LAUNCH(KICK_DRIFT, true);
        else
            BH_TRACER_LAUNCH(KICK_DRIFT, false);
    } else {
        if (off32)
            BH_TRACER_LAUNCH(KICK_ONLY, true);
        else
            BH_TRACER_LAUNCH(KICK_ONLY, false);
    }
#undef BH_TRACER_LAUNCH
}

}  // namespace bh
