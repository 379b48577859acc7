// The radius walk over the flattened quadtree, shared by its two users: bh_find_neighbors
// (neighbors.hip: one lane = one probe), bh_find_groups (groups.hip: one lane = one leaf) and
// bh_find_knn (knn.hip: one lane = one probe with a list of its k best).
// Device code only; every name is local to the including file.
//
// The walk is a stop of cursor_walk.hpp's cursor_walk: one wave-shared pre-order cursor, the node
// record through a scalar load requested one stop ahead, every lane's own decision by ballot.  An
// internal node of depth d is opened by a lane iff dist2(COM, lane) <= (r_lane pad + reach_d)^2,
// where reach_d (neighbor_reach_at) bounds the distance from the node's COM to every leaf under
// it.  The bound holds for a node whose mass lies in the range the COM's rounding analysis covers;
// any other node is opened by every active lane (opening is always safe).  dist2 carries no soft2:
// it is a distance, not a force denominator.  Every path tests NODE_SKIP: a hit is not a term, so
// nothing here may rely on a massless node adding +-0.
#pragma once

#include "bh_device.hpp"
#include "cursor_walk.hpp"

namespace bh {
namespace {

constexpr uint32_t NBR_NONE = 0xFFFFFFFFu;  // no neighbour yet: above every caller index

// What a walk keeps per lane.  NBR_COUNT: the number found.  NBR_NEAREST: that and the smallest
// (d2, caller index).  NBR_PICK: the smallest alone, and the lane shrinks its radius to the best
// d2 so far -- a body farther than the best cannot become the smallest, one at the same d2 still
// can (by index), and `<=` keeps it.  NBR_FILL: the caller indices into the lane's segment.
// NBR_LINK: nothing is kept; the lane's `link` functor is called with the hit leaf's body slot.
// NBR_KNN: the lane's `link` functor is its list of the k best (knn.hip KnnHeap): the leaf of body
// slot link.self is no hit, a hit goes to link.insert(L, d2, caller index), and insert shrinks
// the lane's radius to the k-th best once the list is full -- NBR_PICK's rule for any k.
enum NbrMode {
    NBR_COUNT = 0,
    NBR_NEAREST = 1,
    NBR_PICK = 2,
    NBR_FILL = 3,
    NBR_LINK = 4,
    NBR_KNN = 5
};

struct NbrLane {
    double bx, by;    // the probe
    double r2;        // rj * rj: the exact test's right-hand side
    double rp;        // rj * NEIGHBOR_RADIUS_PAD: the pruning compare's radius
    uint32_t resume;  // active at `cur` iff cur >= resume
    uint32_t found;   // neighbours so far
    double best;      // smallest d2 so far (+inf: none)
    uint32_t bestc;   // its caller index (NBR_NONE: none)
    uint32_t *seg;    // NBR_FILL: the lane's segment of the index list, `room` entries
    uint32_t room;
};

struct NbrNoLink {
    __device__ __forceinline__ void operator()(uint32_t) const {}
};

template <int MODE, bool OFF32, class Link = NbrNoLink>
__device__ __forceinline__ void nbr_walk_wave(const Node *__restrict__ nodes, uint32_t T,
                                              const uint32_t *__restrict__ cidx,
                                              const NeighborReach rc, NbrLane &L,
                                              Link link = Link()) {
    cursor_walk<OFF32, true>(nodes, T, [&](const CursorStop<OFF32> &st)
                                           __attribute__((always_inline)) {
        uint32_t mhi = st.mass_hi;
        asm volatile("" : "+s"(mhi));  // keep the mass-range test scalar
        const uint32_t meta = st.meta, next = st.next, cur = st.cur;
        const bool active = cur >= L.resume;
        const double dx = st.comX - L.bx;
        const double dy = st.comY - L.by;
        const double d2 = dx * dx + dy * dy;
        if (meta & NODE_LEAF) {  // the record is the body: the exact test
            bool hit = active && d2 <= L.r2;
            if constexpr (MODE == NBR_KNN) hit = hit && (meta & NODE_BODY_MASK) != link.self;
            const uint64_t hit_m = __builtin_amdgcn_ballot_w64(hit);
            st.fetch(next);
            if (hit_m != 0ull) {
                if constexpr (MODE == NBR_KNN) {
                    const uint32_t c = cidx[meta & NODE_BODY_MASK];  // wave-uniform address
                    if (hit) link.insert(L, d2, c);
                } else if (MODE == NBR_LINK) {
                    if (hit) link(meta & NODE_BODY_MASK);
                } else {
                    uint32_t c = 0;
                    if (MODE != NBR_COUNT) c = cidx[meta & NODE_BODY_MASK];  // wave-uniform address
                    if (hit) {
                        if (MODE == NBR_FILL && L.found < L.room) L.seg[L.found] = c;
                        if (MODE == NBR_NEAREST || MODE == NBR_PICK) {
                            if (d2 < L.best || (d2 == L.best && c < L.bestc)) {
                                L.best = d2;
                                L.bestc = c;
                                if (MODE == NBR_PICK) {  // correctly rounded sqrt; the pad covers it
                                    L.r2 = d2;
                                    L.rp = __builtin_sqrt(d2) * NEIGHBOR_RADIUS_PAD;
                                }
                            }
                        }
                        ++L.found;
                    }
                }
            }
            return next;
        }
        // internal: prune iff the node's mass is in the covered range and the COM is farther than
        // the padded radius plus the depth's reach; a NaN d2 or threshold never prunes
        const bool covered = (mhi - rc.m_lo) < rc.m_span;
        const double reach = neighbor_reach_at(rc, (int)((meta & NODE_DEPTH2_MASK) >> 1));
        const double t = L.rp + reach;
        const bool prune = covered && d2 > t * t;
        const uint64_t open_m = __builtin_amdgcn_ballot_w64(active && !prune);
        const uint32_t ncur = open_m != 0ull ? cur + 1 : next;  // descend iff some lane opened
        st.fetch(ncur);
        if (active && prune) L.resume = next;  // parked until the cursor has left the subtree
        return ncur;
    });
}

}  // namespace
}  // namespace bh
