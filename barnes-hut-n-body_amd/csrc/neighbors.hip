// Radius query over the flattened quadtree: which bodies lie within r of probe points
// (bh_find_neighbors, include/bh_engine.h).
//
// The candidate set is the leaf sequence of bh_compute_field_direct: every non-empty leaf under no
// mass-0 node (NODE_SKIP records are never entered).  Probe j finds leaf body b iff
//     rj >= 0 && dx*dx + dy*dy <= rj*rj,   dx = x_b - px[j], dy = y_b - py[j]
// in binary64, nothing fused (the build contracts nothing).  A leaf record's comX / comY are its
// body's position, so the test is made on the record itself.
//
// The walk (neighbor_walk.hpp, shared with groups.hip) is a stop of cursor_walk.hpp's shared
// cursor walk, as the field's is: one lane = one probe, one wave-shared pre-order cursor, the node
// record through a scalar load requested one stop ahead, every lane's own decision by ballot.
// The opening criterion has another right-hand side: an internal node of depth d is opened by a
// lane iff dist2(COM, probe) <= (r_lane pad + reach_d)^2, where reach_d (neighbor_reach_at) bounds
// the distance from the node's COM to every leaf under it.  The bound holds for a node whose mass lies in the range the COM's rounding analysis covers; any other node
// is opened by every active lane (opening is always safe).  dist2 carries no soft2: it is a
// distance, not a force denominator.  Every path tests NODE_SKIP: a hit is not a term, so nothing
// here may rely on a massless node adding +-0.
// Every output is an integer, or a minimum under the total order (d2, caller index): no
// floating-point sum, no atomic.  The lists are written by a second, identical walk into the
// segments an exclusive scan of the counts laid out, then sorted per segment.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "bh_device.hpp"
#include "neighbor_walk.hpp"

namespace bh {
namespace {

// Wave v walks the bpw lanes [bpw v, bpw v + bpw); lane q holds probe order[q] and writes its
// results straight to that caller index.  d_T null: no tree was built (no bodies).
template <int MODE, bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_neighbors(
    const Node *__restrict__ nodes, const uint32_t *__restrict__ d_T,
    const uint32_t *__restrict__ cidx, const double *__restrict__ px,
    const double *__restrict__ py, const double *__restrict__ pr, double r,
    const uint32_t *__restrict__ order, int64_t n, NeighborReach rc, int64_t *__restrict__ count,
    int64_t *__restrict__ nearest, double *__restrict__ d2n, const int64_t *__restrict__ offsets,
    uint32_t *__restrict__ idx, uint32_t bpw, uint32_t wpb) {
    const uint32_t v = xcd_run_wave(wpb);
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t q = (int64_t)v * bpw + lane;
    const bool valid = lane < bpw && q < n;
    const int64_t j = valid ? (int64_t)order[q] : 0;  // the probe's caller index
    NbrLane L;
    L.bx = valid ? px[j] : 0.0;
    L.by = valid ? py[j] : 0.0;
    const double rj = valid ? (pr ? pr[j] : r) : -1.0;
    // a NaN coordinate or a NaN or negative radius finds nothing: the lane starts parked, so it
    // never drags the cursor down
    const bool seeks = valid && L.bx == L.bx && L.by == L.by && rj >= 0.0;
    L.r2 = rj * rj;
    L.rp = rj * NEIGHBOR_RADIUS_PAD;
    L.resume = seeks ? 0u : 0xFFFFFFFFu;
    L.found = 0;
    L.best = __builtin_inf();
    L.bestc = NBR_NONE;
    L.seg = nullptr;
    L.room = 0;
    if (MODE == NBR_FILL && valid) {
        const int64_t lo = offsets[j];
        L.seg = idx + lo;
        L.room = (uint32_t)(offsets[j + 1] - lo);
    }
    const uint32_t T = d_T ? __builtin_amdgcn_readfirstlane(*d_T) : 0u;
    nbr_walk_wave<MODE, OFF32>(nodes, T, cidx, rc, L);
    if (!valid) return;
    if (MODE == NBR_COUNT || MODE == NBR_NEAREST) count[j] = (int64_t)L.found;
    if (MODE == NBR_NEAREST || MODE == NBR_PICK) {
        nearest[j] = L.bestc == NBR_NONE ? (int64_t)-1 : (int64_t)L.bestc;
        d2n[j] = L.best;
    }
}

constexpr int WID_TB = 256;
__global__ __launch_bounds__(WID_TB) void k_neighbors_widen(int64_t n,
                                                            const uint32_t *__restrict__ in,
                                                            int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * WID_TB + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i];
}

template <int MODE>
void nbr_launch(const Node *nodes, size_t node_cap, const uint32_t *d_T, const uint32_t *cidx,
                const double *px, const double *py, const double *pr, double r,
                const uint32_t *order, int64_t n, const NeighborReach &rc, int64_t *count,
                int64_t *nearest, double *d2n, const int64_t *offsets, uint32_t *idx,
                hipStream_t s) {
    if (n <= 0) return;
    const WalkShape w = walk_shape(n);
    if (node_off32(node_cap))
        k_neighbors<MODE, true><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, cidx, px, py, pr, r,
                                                              order, n, rc, count, nearest, d2n,
                                                              offsets, idx, w.bpw, w.wpb);
    else
        k_neighbors<MODE, false><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, cidx, px, py, pr, r,
                                                               order, n, rc, count, nearest, d2n,
                                                               offsets, idx, w.bpw, w.wpb);
}

}  // namespace

// DESIGN.md §17 derives the terms.  A leaf lies in its cell and in every ancestor's (BHA:126 tests
// containment at every insert, also after a jitter), and a node's COM is a positive-weight mean
// of points of its cell, so in exact arithmetic their distance is at most the cell's diagonal.
NeighborReach neighbor_reach_terms(const Geometry &g) {
    const double margin = NEIGHBOR_RADIUS_PAD;  // the same 2^-40, far above any rounding below
    const double sqrt2 = 1.4142135623730951;
    // largest |coordinate| of a point of the root cell
    const double ext = std::fmax(std::fabs(g.root_cx), std::fabs(g.root_cy)) + g.root_h;
    NeighborReach rc;
    rc.diag0 = 2.0 * sqrt2 * g.root_h * margin;
    // let.hip's allowance for the jitter, 2 x 2e-3 per axis (not needed by the containment
    // argument; it keeps a body covered should a replay ever leave a moved body in place), and the
    // COM's own rounding: at most 10 ulp of ext per axis while nothing over- or underflows
    const double jitter = sqrt2 * (2.0 * 2e-3);
    const double com = sqrt2 * 16.0 * 0x1p-53 * ext;
    rc.slack = (jitter + com) * margin;
    // node masses the COM bound covers: from 2^-900 (a product or partial sum that goes subnormal
    // then errs by at most 2^-1074 / 2^-900) up to the power of two below DBL_MAX / (4 ext) (no
    // partial sum of comX * mass overflows); both powers of two, so the compare of the high words
    // is the compare of the values
    int ex = 0;
    (void)std::frexp(4.0 * ext, &ex);  // 4 ext < 2^ex
    const uint64_t lo = (uint64_t)__builtin_bit_cast(int64_t, std::ldexp(1.0, -900));
    const uint64_t hi = (uint64_t)__builtin_bit_cast(int64_t, std::ldexp(1.0, 1023 - ex));
    rc.m_lo = (uint32_t)(lo >> 32);
    rc.m_span = (uint32_t)(hi >> 32) - rc.m_lo;
    return rc;
}

void neighbors_count(const Node *nodes, size_t node_cap, const uint32_t *d_T, const uint32_t *cidx,
                     const double *px, const double *py, const double *pr, double r,
                     const uint32_t *order, int64_t n, const NeighborReach &rc, int64_t *count,
                     int64_t *nearest, double *d2n, hipStream_t s) {
    if (!count)
        nbr_launch<NBR_PICK>(nodes, node_cap, d_T, cidx, px, py, pr, r, order, n, rc, nullptr,
                             nearest, d2n, nullptr, nullptr, s);
    else if (nearest)
        nbr_launch<NBR_NEAREST>(nodes, node_cap, d_T, cidx, px, py, pr, r, order, n, rc, count,
                                nearest, d2n, nullptr, nullptr, s);
    else
        nbr_launch<NBR_COUNT>(nodes, node_cap, d_T, cidx, px, py, pr, r, order, n, rc, count,
                              nullptr, nullptr, nullptr, nullptr, s);
}

size_t neighbors_scan_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const int64_t *)nullptr, (int64_t *)nullptr,
                                  (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>());
    return bytes;
}

hipError_t neighbors_offsets(int64_t n, const int64_t *count, int64_t *offsets, void *scratch,
                             size_t scratch_bytes, hipStream_t s) {
    size_t bytes = scratch_bytes;
    return rocprim::exclusive_scan(scratch, bytes, count, offsets, (int64_t)0, (size_t)(n + 1),
                                   rocprim::plus<int64_t>(), s);
}

void neighbors_fill(const Node *nodes, size_t node_cap, const uint32_t *d_T, const uint32_t *cidx,
                    const double *px, const double *py, const double *pr, double r,
                    const uint32_t *order, int64_t n, const NeighborReach &rc,
                    const int64_t *offsets, uint32_t *idx, hipStream_t s) {
    nbr_launch<NBR_FILL>(nodes, node_cap, d_T, cidx, px, py, pr, r, order, n, rc, nullptr, nullptr,
                         nullptr, offsets, idx, s);
}

hipError_t neighbors_sort(int64_t total, int64_t n, const int64_t *offsets, uint32_t *idx,
                          uint32_t *idx_s, int bits, int64_t *out, void *scratch,
                          size_t &scratch_bytes, hipStream_t s) {
    if (scratch_bytes == 0) {
        hipError_t st = rocprim::segmented_radix_sort_keys(
            nullptr, scratch_bytes, idx, idx_s, (unsigned)total, (unsigned)n, offsets, offsets + 1,
            0u, (unsigned)bits);
        if (scratch_bytes == 0) scratch_bytes = 1;
        return st;
    }
    size_t bytes = scratch_bytes;
    hipError_t st = rocprim::segmented_radix_sort_keys(scratch, bytes, idx, idx_s, (unsigned)total,
                                                       (unsigned)n, offsets, offsets + 1, 0u,
                                                       (unsigned)bits, s);
    if (st != hipSuccess) return st;
    k_neighbors_widen<<<(unsigned)((total + WID_TB - 1) / WID_TB), WID_TB, 0, s>>>(total, idx_s,
                                                                                   out);
    return hipGetLastError();
}

}  // namespace bh
