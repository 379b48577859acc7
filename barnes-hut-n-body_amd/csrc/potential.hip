// Gravitational potential over the flattened quadtree, and the deterministic reductions of the
// global diagnostics (bh_compute_potential / bh_compute_diagnostics, include/bh_engine.h).
//
// Body b visits exactly the nodes accumulateForce visits for it (BHA:215-239): massless nodes
// are skipped (BHA:216), the own leaf is skipped by identity (BHA:219), an internal node is taken
// iff s2 < theta2 * dist2 (BHA:226-228), else its children are visited in order.  Every taken
// node adds, in that pre-order,
//     dx = comX - b.x;  dy = comY - b.y;  r2 = dx*dx + dy*dy + soft2
//     s += mass * (1.0 / sqrt(r2))                   (IEEE sqrt and divide, s from +0.0)
// and phi_b = -(G * s).  An accepted cell that contains b includes b's own mass, exactly as the
// force of that cell does; at theta = 0 nothing is accepted and phi is the exact softened pair
// potential over the bodies in the tree (direct.hip runs that case as an all-pairs kernel).
//
// The walk is the probe walk of cursor_walk.hpp (probe_walk, shared with field.hip) for a lane
// that owns a slot: one lane = one body, one wave-shared pre-order cursor, every lane's own
// criterion by ballot.  The term is a subset of the force term's arithmetic: one sqrt and one
// reciprocal.  Unlike the force, the own leaf's term m / sqrt(soft2) is not zero, so leaves need
// the identity test.  s is never -0.0: it starts at +0.0 and x + (+-0) keeps x.
#include "bh_device.hpp"
#include "cursor_walk.hpp"
#include "diag_sum.hpp"

namespace bh {
namespace {

// Wave v walks the lanes [64 v, 64 v + 64); lane q holds body slot lanes[q] (or q); phi is
// written by slot.  A tombstone (CIDX_DEAD) does not walk and gets phi = 0.
template <bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_potential(const Node *__restrict__ nodes,
                                                            const uint32_t *__restrict__ d_T,
                                                            const double *__restrict__ x,
                                                            const double *__restrict__ y,
                                                            const uint32_t *__restrict__ cidx,
                                                            int64_t n, ForceParams fp, double s2root,
                                                            double *__restrict__ phi,
                                                            const uint32_t *__restrict__ lanes,
                                                            uint32_t wpb) {
    const uint32_t v = xcd_run_wave(wpb);
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t q = (int64_t)v * TB + lane;
    const uint32_t lp = lanes && q < n ? lanes[q] : (uint32_t)q;
    const bool valid = q < n && (!lanes || (lp != LANE_IDLE && (int64_t)lp < n));
    const int64_t p = lanes ? (int64_t)lp : q;  // the body's slot
    const bool walks = valid && !(cidx[p] & CIDX_DEAD);
    const double bx = valid ? x[p] : 0.0;
    const double by = valid ? y[p] : 0.0;
    const double soft2 = fp.soft2, theta2 = fp.theta2;
    const uint32_t resume = walks ? 0u : 0xFFFFFFFFu;  // active at `cur` iff cur >= resume
    const uint32_t T = __builtin_amdgcn_readfirstlane(*d_T);
    const bool fast =
        fast_s2_ok(s2root) && __ballot(walks && !lane_fast_ok(bx, by, soft2)) == 0ull;
    double s = 0.0, fx = 0.0, fy = 0.0;  // (no force is summed)
    if (fast)
        probe_walk<true, OFF32, true, PROBE_POT>(nodes, T, bx, by, 0.0, soft2, theta2, s2root,
                                                 (uint32_t)p, resume, fx, fy, s);
    else
        probe_walk<false, OFF32, true, PROBE_POT>(nodes, T, bx, by, 0.0, soft2, theta2, s2root,
                                                  (uint32_t)p, resume, fx, fy, s);
    if (!valid) return;
    phi[p] = walks ? -(fp.G * s) : 0.0;
}

// ---- global diagnostics: fixed-order reductions, no floating-point atomics ----------------
// (the partition, the per-thread order and the LDS tree are diag_sum.hpp's, shared with the step
// log's records)
__global__ __launch_bounds__(DIAG_TB) void k_diag_partial(int64_t n, int64_t chunk,
                                                          const double *__restrict__ x,
                                                          const double *__restrict__ y,
                                                          const double *__restrict__ vx,
                                                          const double *__restrict__ vy,
                                                          const double *__restrict__ m,
                                                          const double *__restrict__ phi,
                                                          double *__restrict__ part) {
    __shared__ double lds[DIAG_K][DIAG_TB];
    diag_partial_block((int)blockIdx.x, n, chunk, x, y, vx, vy, m, phi, part, lds);
}

__global__ __launch_bounds__(DIAG_TB) void k_diag_final(int blocks, const double *__restrict__ part,
                                                        double *__restrict__ out) {
    __shared__ double lds[DIAG_K][DIAG_TB];
    diag_final_block(blocks, part, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < DIAG_K; ++k) out[k] = lds[k][0];
}

}  // namespace

void potential_walk(const Node *nodes, size_t node_cap, const uint32_t *d_T, const double *x,
                    const double *y, const uint32_t *cidx, int64_t n, const Geometry &g,
                    const ForceParams &fp, double *phi, const uint32_t *lanes, hipStream_t s) {
    if (n <= 0) return;
    const WalkShape w = walk_shape(n, true);  // (whole waves: a lane map's groups are 64 lanes)
    if (node_off32(node_cap))
        k_potential<true><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, x, y, cidx, n, fp, g.s2[0],
                                                        phi, lanes, w.wpb);
    else
        k_potential<false><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, x, y, cidx, n, fp, g.s2[0],
                                                         phi, lanes, w.wpb);
}

size_t diag_partial_doubles() { return (size_t)(DIAG_MAX_BLOCKS + 1) * DIAG_K; }

void diag_reduce(int64_t n, const double *x, const double *y, const double *vx, const double *vy,
                 const double *m, const double *phi, double *part, double *out8, hipStream_t s) {
    const DiagPartition dp = diag_partition(n);
    const int64_t chunk = dp.chunk;
    const int blocks = dp.blocks;
    k_diag_partial<<<blocks, DIAG_TB, 0, s>>>(n, chunk, x, y, vx, vy, m, phi, part);
    k_diag_final<<<1, DIAG_TB, 0, s>>>(blocks, part, out8);
}

}  // namespace bh
