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
// The walk is traverse.hip's: one lane = one body, one wave-shared pre-order cursor, the node
// record through a scalar load requested one stop ahead, every lane's own criterion by ballot.
// The term is a subset of the force term's arithmetic: one sqrt and one reciprocal.  Unlike the
// force, the own leaf's term m / sqrt(soft2) is not zero, so leaves need the identity test.
#include "bh_device.hpp"
#include "diag_sum.hpp"
#include "fastmath.hpp"

namespace bh {
namespace {

constexpr int TB = 64;
constexpr int MAX_WPB = 8;           // waves per workgroup (traverse.hip waves_per_group)
constexpr uint32_t POT_XCD_RUN = 64; // consecutive waves per XCD (traverse.hip BH_TRAV_XCD_RUN)
static_assert(POT_XCD_RUN % MAX_WPB == 0, "an XCD run holds whole workgroups");

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// Node record through an explicit scalar load whose wait is placed by hand (traverse.hip nload).
__device__ __forceinline__ u32x8 nload(const Node *p) {
    u32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(v) : "s"(p) : "memory");
    return v;
}
__device__ __forceinline__ u32x8 nload_off(const Node *base, uint32_t idx) {
    u32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(v) : "s"(base), "s"(idx << 5) : "memory");
    return v;
}
__device__ __forceinline__ void nwait(u32x8 &v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v)); }
__device__ __forceinline__ double as_f64(uint32_t lo, uint32_t hi) {
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// FAST: the wave's operands are inside the range guards of fastmath.hpp (fast_s2_ok,
// lane_fast_ok), where the seeded sqrt / reciprocal sequences equal the IEEE operations and the
// criterion's s2 is formed by an exponent subtraction.  A massless node then needs no test: it
// carries the leaf flag (bh_device.hpp NODE_SKIP), so the cursor moves past its subtree, and its
// term mass * invR is an exact +-0 (invR finite) that leaves s -- never -0.0 -- unchanged.
template <bool FAST, bool OFF32>
__device__ __forceinline__ void pot_walk(const Node *__restrict__ nodes, uint32_t T, double bx,
                                         double by, double soft2, double theta2, double s2root,
                                         uint32_t self, uint32_t resume, double &s) {
    uint32_t cur = 0;
    // one iteration on record `rec`; the next record is requested into `nrec` (the node array
    // has slack beyond T, so loading node T is harmless)
    auto iter = [&](const u32x8 &rec, u32x8 &nrec) __attribute__((always_inline)) {
        const double comX = as_f64(rec[0], rec[1]), comY = as_f64(rec[2], rec[3]);
        const double mass = as_f64(rec[4], rec[5]);
        uint32_t meta = rec[7];
        asm volatile("" : "+s"(meta));  // keep the flag tests scalar
        uint32_t next = rec[6];
        next = next > cur ? next : cur + 1;  // structural guard: the cursor always advances
        if (!FAST && (meta & NODE_SKIP)) {   // mass == 0.0 (BHA:216): not visited
            cur = next;
            nrec = OFF32 ? nload_off(nodes, cur) : nload(nodes + cur);
            nwait(nrec);
            return;
        }
        const uint64_t act_m = __builtin_amdgcn_ballot_w64(cur >= resume);
        const double dx = comX - bx;
        const double dy = comY - by;
        const double d2 = dx * dx + dy * dy + soft2;
        uint64_t contrib_m, open_m;  // lanes that take / open this node
        if (meta & NODE_LEAF) {      // BHA:217-221: the own leaf is skipped by identity
            contrib_m = act_m & __builtin_amdgcn_ballot_w64((meta & NODE_BODY_MASK) != self);
            open_m = 0;
        } else {  // BHA:226-228, decided exactly as traverse.hip's walk decides it
            uint64_t acc_m;
            if (FAST) {
                const uint64_t s2b = (uint64_t)__double_as_longlong(s2root) -
                                     ((uint64_t)(meta & NODE_DEPTH2_MASK) << 52);
                acc_m = __builtin_amdgcn_ballot_w64(__longlong_as_double((long long)s2b) <
                                                    theta2 * d2);
            } else {
                const double t2 = __builtin_ldexp(theta2 * d2, (int)(meta & NODE_DEPTH2_MASK));
                acc_m = __builtin_amdgcn_ballot_w64(s2root < t2);
            }
            contrib_m = act_m & acc_m;
            open_m = act_m & ~acc_m;
        }
        const uint32_t ncur = open_m != 0ull ? cur + 1 : next;  // descend iff some lane opened
        nrec = OFF32 ? nload_off(nodes, ncur) : nload(nodes + ncur);
        if (__builtin_amdgcn_inverse_ballot_w64(contrib_m)) {
            double invR;
            if (FAST) {
                double h;
                const double r = sqrt_rn_inrange_h(d2, h);
                invR = rcp_rn_seeded(r, h + h);
            } else {
                invR = 1.0 / sqrt(d2);
            }
            s += mass * invR;
            resume = next;
        }
        nwait(nrec);
        cur = ncur;
    };
    if (T == 0) return;  // no body inside the root cell: an empty tree
    u32x8 r0 = nload(nodes), r1;
    nwait(r0);
    while (true) {
        iter(r0, r1);
        if (cur >= T) break;
        iter(r1, r0);
        if (cur >= T) break;
    }
}

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
    uint32_t b = blockIdx.x;  // runs of POT_XCD_RUN consecutive waves per XCD (bh_device.hpp)
    {
        const uint32_t C = POT_XCD_RUN / wpb, G = 8 * C, full = gridDim.x / G;
        if (b < full * G) b = (b / 8 / C) * G + (b % 8) * C + (b / 8) % C;
    }
    const uint32_t v = b * wpb + (threadIdx.x >> 6);
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
    double s = 0.0;
    if (fast)
        pot_walk<true, OFF32>(nodes, T, bx, by, soft2, theta2, s2root, (uint32_t)p, resume, s);
    else
        pot_walk<false, OFF32>(nodes, T, bx, by, soft2, theta2, s2root, (uint32_t)p, resume, s);
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
    const bool off32 = node_cap * sizeof(Node) < (size_t(1) << 32);
    const uint32_t waves = (uint32_t)((n + TB - 1) / TB);
    const uint32_t wpb = waves >= 8192 ? 4u : waves >= 1024 ? 8u : 1u;  // (as k_traverse)
    const unsigned grid = (waves + wpb - 1) / wpb;
    if (off32)
        k_potential<true><<<grid, TB * wpb, 0, s>>>(nodes, d_T, x, y, cidx, n, fp, g.s2[0], phi,
                                                    lanes, wpb);
    else
        k_potential<false><<<grid, TB * wpb, 0, s>>>(nodes, d_T, x, y, cidx, n, fp, g.s2[0], phi,
                                                     lanes, wpb);
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
