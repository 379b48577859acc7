// The wave-shared cursor walk over the flattened quadtree: what the force walk (traverse.hip
// walk), the probe walk of the potential and the field (probe_walk below: potential.hip,
// field.hip) and the radius walk (neighbor_walk.hpp: neighbors.hip, groups.hip) have in common.
// Device code only; every name is local to the including file.
//
// One lane = one body or probe, one wave = one pre-order cursor.  The node record is wave-uniform
// (one 32-byte scalar load serves 64 lanes); every lane decides for itself at every stop, and the
// cursor descends (cur + 1) iff at least one lane opened the node, else it leaves the subtree
// (cur = next).  A lane that is done with a subtree parks itself until the cursor has left it
// (resume = next; active at `cur` iff cur >= resume).  What a lane decides and what it keeps is
// the walk's own "stop" (cursor_walk below); the record's way from memory, the loop and the
// launch's wave numbering are here, once.
#pragma once

#include "bh_device.hpp"
#include "fastmath.hpp"

namespace bh {
namespace {

constexpr int TB = 64;  // one wave per workgroup: finest dispatch granularity (C4 -1.5 %, C3 -0.5 %)
// Waves per workgroup of a walking kernel: up to MAX_WPB, chosen per launch (traverse.hip
// waves_per_group).  A workgroup's waves share one CU and its scalar data cache, and neighbouring
// waves walk nearly the same node records.
constexpr int MAX_WPB = 8;

// Workgroups in runs of BH_TRAV_XCD_RUN consecutive waves per XCD (bh_device.hpp xcd_block):
// neighbouring waves walk nearly the same nodes, so a run shares its XCD's L2 (C3 -1.5 % at runs
// of 32..512 against the round-robin default).
#ifndef BH_TRAV_XCD_RUN
#define BH_TRAV_XCD_RUN 64
#endif
static_assert(BH_TRAV_XCD_RUN % MAX_WPB == 0, "an XCD run holds whole workgroups");
// Workgroups of one remapped group (8 XCDs x one run each) and the whole groups of a grid: the
// tail past them keeps its dispatch order (xcd_run_wave, bh_launch_plan).
__host__ __device__ constexpr uint32_t xcd_group_blocks(uint32_t wpb) {
    return 8u * (BH_TRAV_XCD_RUN / wpb);
}
__host__ __device__ constexpr uint32_t xcd_full_groups(uint32_t groups, uint32_t wpb) {
    return groups / xcd_group_blocks(wpb);
}
// The wave this wave walks as, in a launch of wpb-wave workgroups: xcd_block() with runs of
// BH_TRAV_XCD_RUN / wpb workgroups (= BH_TRAV_XCD_RUN waves).
__device__ __forceinline__ uint32_t xcd_run_wave(uint32_t wpb) {
    uint32_t b = blockIdx.x;
    const uint32_t C = BH_TRAV_XCD_RUN / wpb, G = xcd_group_blocks(wpb);
    const uint32_t full = xcd_full_groups(gridDim.x, wpb);
    if (b < full * G) b = (b / 8 / C) * G + (b % 8) * C + (b / 8) % C;
    return b * wpb + (threadIdx.x >> 6);
}

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// Node record through an explicit scalar load whose wait is placed by hand (nwait): the next
// record is requested as soon as the cursor decision is made and waited for only after the
// stop's block, so its latency hides behind that block's fp64 work.  (The compiler would
// sink a plain load below the block, to its first use.)
__device__ __forceinline__ u32x8 nload(const Node *p) {
    u32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(v) : "s"(p) : "memory");
    return v;
}
// Same, addressed as base + 32-bit byte offset (s_load's SGPR offset): one shift per
// iteration instead of a 64-bit address computation.  Only for node arrays below 4 GiB
// (bh_device.hpp node_off32).
__device__ __forceinline__ u32x8 nload_off(const Node *base, uint32_t idx) {
    u32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(v) : "s"(base), "s"(idx << 5) : "memory");
    return v;
}
__device__ __forceinline__ void nwait(u32x8 &v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v)); }
__device__ __forceinline__ double as_f64(uint32_t lo, uint32_t hi) {
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// One stop of the cursor: the decoded record, all wave-uniform, and the request for the next one.
template <bool OFF32>
struct CursorStop {
    double comX, comY, mass;
    uint32_t mass_hi;  // the mass's high word (sign, exponent: range tests on the scalar unit)
    uint32_t meta;     // NODE_* (bh_device.hpp)
    uint32_t next;     // past the node's subtree; always beyond cur
    uint32_t cur;      // the node's index
    const Node *nodes;
    u32x8 &nrec;
    // Requests record `ncur`, the stop's choice of the next cursor; the walk waits for it after
    // the stop has returned.  The only place a walk picks between the two address forms.
    __device__ __forceinline__ void fetch(uint32_t ncur) const {
        nrec = OFF32 ? nload_off(nodes, ncur) : nload(nodes + ncur);
    }
};

// Walks nodes [0, T) from the root.  At every node the cursor reaches, stop(st) decides the
// next cursor -- st.cur + 1 to descend, st.next to leave the subtree --, calls st.fetch(it) as
// soon as it is known, does its block and returns it; the wait for the record comes after.
// SKIP: a massless node (NODE_SKIP, BHA:216) is not a stop at all.  A walk whose terms at such a
// node are exact +-0 needs no test (it carries the leaf flag too, so no lane opens it).
template <bool OFF32, bool SKIP, class Stop>
__device__ __forceinline__ void cursor_walk(const Node *__restrict__ nodes, uint32_t T, Stop stop) {
    uint32_t cur = 0;
    // one iteration on record `rec`; the next record is requested into `nrec`.  The loop body
    // is unrolled twice with the two records swapping roles (no SGPR copies per iteration).
    // Loading node T (past the last one) is harmless: the node array has slack beyond T.
    auto iter = [&](const u32x8 &rec, u32x8 &nrec) __attribute__((always_inline)) {
        CursorStop<OFF32> st{as_f64(rec[0], rec[1]), as_f64(rec[2], rec[3]),
                             as_f64(rec[4], rec[5]), rec[5], rec[7], rec[6], cur, nodes, nrec};
        asm volatile("" : "+s"(st.meta));  // keep the flag tests scalar (s_bitcmp)
        st.next = st.next > cur ? st.next : cur + 1;  // structural guard: the cursor always advances
        if (SKIP && (st.meta & NODE_SKIP)) {  // (its own request and wait: the paths stay apart)
            cur = st.next;
            st.fetch(cur);
            nwait(nrec);
            return;
        }
        const uint32_t ncur = stop(st);
        nwait(nrec);
        cur = ncur;
    };
    if (T == 0) return;  // no body inside the root cell: an empty tree
    u32x8 r0 = nload(nodes), r1;
    nwait(r0);
    // (a `while (cur < T)` head with one exit test in the middle made the compiler keep a dead
    // v_readfirstlane per two stops)
    while (true) {
        iter(r0, r1);
        if (cur >= T) break;
        iter(r1, r0);
        if (cur >= T) break;
    }
}

// ---- the probe walk: potential and field ---------------------------------------------------
// A lane is a point (bx, by) that visits exactly the nodes accumulateForce visits for a body
// there (BHA:215-239): massless nodes are skipped (BHA:216), an internal node is taken iff
// s2 < theta2 * dist2 (BHA:226-228), else its children are visited in order.
// OWN: the lane is the body in slot `self`, whose own leaf is skipped by identity (BHA:219) --
// its potential term m / sqrt(soft2) is not zero.  Without it the lane is in no leaf and takes
// every non-empty one: no path compares a leaf with anything, and no term is ever excused.
// SUMS: what a taken node adds, in pre-order from +0.0, nothing fused:
//     dx = comX - bx;  dy = comY - by;  r2 = dx*dx + dy*dy + soft2;  invR = 1.0 / sqrt(r2)
//     PROBE_FORCE:  invR2 = 1.0 / r2;  f = Gm * mass * invR2                       (BHA:250-259)
//                   fx += f * dx * invR;  fy += f * dy * invR
//     PROBE_POT:    s += mass * invR                     (bh_compute_potential's term)
// FAST: the wave's operands are inside the range guards of fastmath.hpp (fast_s2_ok,
// lane_fast_ok) and every lane's Gm is finite: the seeded sqrt / reciprocal sequences equal the
// IEEE operations and the criterion's s2 is formed by an exponent subtraction.  A massless node
// then needs no test: it carries the leaf flag (bh_device.hpp NODE_SKIP), so the cursor moves past
// its subtree, and its terms -- f = Gm * 0 * invR2, 0 * invR, all factors finite -- are exact +-0
// that leave the sums (from +0.0, never -0.0) unchanged.  lane_self_ok has no counterpart: a
// coincident body's term is owed, whatever it is, and both paths compute it with the same
// operations.
enum ProbeSums { PROBE_FORCE = 1, PROBE_POT = 2, PROBE_BOTH = 3 };

template <bool FAST, bool OFF32, bool OWN, int SUMS>
__device__ __forceinline__ void probe_walk(const Node *__restrict__ nodes, uint32_t T, double bx,
                                           double by, double Gm, double soft2, double theta2,
                                           double s2root, uint32_t self, uint32_t resume,
                                           double &fx, double &fy, double &s) {
    cursor_walk<OFF32, !FAST>(nodes, T, [&](const CursorStop<OFF32> &st)
                                            __attribute__((always_inline)) {
        const uint64_t act_m = __builtin_amdgcn_ballot_w64(st.cur >= resume);
        const double dx = st.comX - bx;  // BHA:223-225 == BHA:251-253
        const double dy = st.comY - by;
        const double d2 = dx * dx + dy * dy + soft2;
        uint64_t contrib_m, open_m;  // lanes that take / open this node
        if (st.meta & NODE_LEAF) {   // BHA:217-221
            contrib_m = OWN ? act_m & __builtin_amdgcn_ballot_w64((st.meta & NODE_BODY_MASK) != self)
                            : act_m;
            open_m = 0;
        } else {  // BHA:226-228: s2 = s2root * 4^-d exactly (traverse.hip walk)
            uint64_t acc_m;
            if (FAST) {
                const uint64_t s2b = (uint64_t)__double_as_longlong(s2root) -
                                     ((uint64_t)(st.meta & NODE_DEPTH2_MASK) << 52);
                acc_m = __builtin_amdgcn_ballot_w64(__longlong_as_double((long long)s2b) <
                                                    theta2 * d2);
            } else {
                const double t2 = __builtin_ldexp(theta2 * d2, (int)(st.meta & NODE_DEPTH2_MASK));
                acc_m = __builtin_amdgcn_ballot_w64(s2root < t2);
            }
            contrib_m = act_m & acc_m;
            open_m = act_m & ~acc_m;
        }
        const uint32_t ncur = open_m != 0ull ? st.cur + 1 : st.next;  // descend iff some lane opened
        st.fetch(ncur);
        if (__builtin_amdgcn_inverse_ballot_w64(contrib_m)) {  // order as written
            double invR, invR2 = 0.0;
            if (FAST) {
                double h;
                const double r = sqrt_rn_inrange_h(d2, h);
                invR = rcp_rn_seeded(r, h + h);
                if (SUMS & PROBE_FORCE) invR2 = rcp_rn_seeded(d2, invR * invR);
            } else {
                invR = 1.0 / sqrt(d2);
                if (SUMS & PROBE_FORCE) invR2 = 1.0 / d2;
            }
            if (SUMS & PROBE_FORCE) {
                const double f = Gm * st.mass * invR2;
                fx += f * dx * invR;
                fy += f * dy * invR;
            }
            if (SUMS & PROBE_POT) s += st.mass * invR;
            resume = st.next;
        }
        return ncur;
    });
}

}  // namespace
}  // namespace bh
