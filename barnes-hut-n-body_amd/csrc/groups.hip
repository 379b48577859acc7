// Friends-of-friends groups of the bodies in the tree (bh_find_groups, include/bh_engine.h;
// DESIGN.md §18).
//
// The candidate set S is the leaf sequence of leaf_list_build: every non-empty leaf under no
// mass-0 node.  Bodies a != b of S are linked iff dx*dx + dy*dy <= link*link in binary64, nothing
// fused; a group is a connected component of that relation, its label the smallest caller index
// among its members.
//
// The link walk is bh_find_neighbors' (neighbor_walk.hpp, mode NBR_LINK): one lane = one leaf of
// the leaf sequence, which is in pre-order = Morton order, so a wave's lanes are neighbours in
// space.  The lane's position is the leaf record's own (x, y) -- the bits the walk meets again
// as that leaf's node record -- so x_a - x_b is the exact negation of x_b - x_a, d2 is the same
// from both ends and the relation is symmetric bit for bit.  A lane therefore acts only on hits
// whose body slot is below its own: the other end of every such pair is skipped by its own lane,
// and a hit on itself is nothing.  The pruning compare is conservative from either end, so it
// changes the work, never the pairs found.
//
// The union-find: parent[] holds one 32-bit index per body slot, parent[s] = s at the start.
//
//  1. Memory model.  Waves of one kernel on different XCDs do not see each other's plain stores
//     (the L2s are not coherent with each other), so in the link kernel every read of parent[]
//     is a relaxed agent-scope atomic load or the value an atomic returned, and every write is an
//     agent-scope atomic (a compare-and-swap that hooks a root, a min that shortens a path).
//     parent[s] only ever decreases and never leaves s's component, so a stale value is an older,
//     higher ancestor: following it costs steps, not correctness.  The one write that decides
//     something -- hooking root a under b < a -- is a compare-and-swap that expects parent[a] == a,
//     so it succeeds only if a is still a root at that moment; when it fails, the value it
//     returned (lower than a) is where the loop goes on.  Nothing is ever re-read through a plain
//     load in the hope that it has changed.
//  2. Termination.  The structure is lock-free: no lane waits for another lane, wave or workgroup;
//     there is no lock, no ticket, no barrier between workgroups.  uf_find follows strictly
//     decreasing indices (it stops at the first index that does not decrease).  uf_union retries
//     only after a compare-and-swap failed because someone else lowered parent[a], and then goes
//     on from that strictly lower value; so each loop is bounded by the number of slots.  The
//     walk keeps its structural guard: the cursor always advances.
//
// Flattening, labels and the catalogue run in later kernels, where the kernel boundary has made
// every write visible: each leaf finds its root, the component's smallest caller index is an
// integer atomic min, the keys (label, caller) are sorted once by rocprim's radix sort over the
// bits N needs, run heads give label, count and first, a scan and a compaction apply min_members,
// and the sums are made in two fixed-order levels (256-member blocks, then the blocks of a group).
// No floating-point atomic anywhere; every output is an integer or a sum in a fixed order.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bh_device.hpp"
#include "neighbor_walk.hpp"

namespace bh {
namespace {

constexpr int GTB = 256;
constexpr uint32_t GRP_BLOCK = 256;  // members per block of a group's two-level sums
constexpr int SUM_TB = 1024;

typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this lane can see it: a slot r with parent[r] == r when it was
// read.  Strictly decreasing indices; paths are halved on the way by an atomic min.
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    while (true) {
        const uint32_t p = uf_load(parent + x);
        if (p >= x) return x;  // a root (p > x never happens: parents only decrease)
        const uint32_t g = uf_load(parent + p);
        if (g >= p) return p;
        (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;  // g < p < x
    }
}

// Joins the trees of a and b; returns a slot of the joined tree no higher than either root seen.
__device__ __forceinline__ uint32_t uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t expect = a;  // hook root a under the lower b, iff a is still a root
        if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return b;
        if (expect >= a) return b;  // (never: a failed exchange returns a lower parent)
        a = expect;                 // someone hooked a first: go on from where it points
    }
}

// The action of the link walk at a hit leaf of body slot b: a union with the lane's own tree,
// for the pairs whose other end is the lower slot.
struct GroupLink {
    uint32_t *parent;
    uint32_t self;  // the lane's body slot
    uint32_t root;  // a slot of its tree, as low as the lane has seen
    __device__ __forceinline__ void operator()(uint32_t b) {
        if (b < self) root = uf_union(parent, root, b);
    }
};

__global__ __launch_bounds__(GTB) void k_groups_init(int64_t n, uint32_t *__restrict__ parent,
                                                     uint32_t *__restrict__ minc,
                                                     int64_t *__restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i >= n) return;
    parent[i] = (uint32_t)i;
    minc[i] = 0xFFFFFFFFu;
    label[i] = -1;
}

// Wave v walks the leaves [bpw v, bpw v + bpw) of the leaf sequence; lanes beyond the device-side
// leaf count idle, and a wave of such lanes leaves at once.
template <bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_groups_link(
    const Node *__restrict__ nodes, const uint32_t *__restrict__ d_T,
    const double *__restrict__ leaves, const uint32_t *__restrict__ d_count, double link,
    NeighborReach rc, uint32_t *parent, uint32_t bpw, uint32_t wpb) {
    const uint32_t v = xcd_run_wave(wpb);
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t q = (int64_t)v * bpw + lane;
    const uint32_t nl = __builtin_amdgcn_readfirstlane(*d_count);
    const bool valid = lane < bpw && q < (int64_t)nl;
    if (__builtin_amdgcn_ballot_w64(valid) == 0ull) return;
    double4_t rec = {0.0, 0.0, 0.0, 0.0};
    if (valid) rec = reinterpret_cast<const double4_t *>(leaves)[q];
    NbrLane L;
    L.bx = rec.x;
    L.by = rec.y;
    L.r2 = link * link;
    L.rp = link * NEIGHBOR_RADIUS_PAD;
    L.resume = valid ? 0u : 0xFFFFFFFFu;  // an idle lane never drags the cursor down
    L.found = 0;
    L.best = 0.0;
    L.bestc = NBR_NONE;
    L.seg = nullptr;
    L.room = 0;
    GroupLink act;
    act.parent = parent;
    act.self = valid ? (uint32_t)__double_as_longlong(rec.w) : 0u;
    act.root = act.self;
    const uint32_t T = __builtin_amdgcn_readfirstlane(*d_T);
    nbr_walk_wave<NBR_LINK, OFF32>(nodes, T, nullptr, rc, L, act);
}

// Every leaf finds its root; the component's smallest caller index by an integer atomic min.
__global__ __launch_bounds__(GTB) void k_groups_root(const double *__restrict__ leaves,
                                                     const uint32_t *__restrict__ d_count,
                                                     const uint32_t *__restrict__ cidx,
                                                     uint32_t *parent,
                                                     uint32_t *__restrict__ rootof,
                                                     uint32_t *minc) {
    const uint32_t i = blockIdx.x * GTB + threadIdx.x;
    if (i >= *d_count) return;
    const uint32_t slot = (uint32_t)__double_as_longlong(leaves[4 * (size_t)i + 3]);
    const uint32_t r = uf_find(parent, slot);
    rootof[i] = r;
    (void)__hip_atomic_fetch_min(minc + r, cidx[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// label[caller] for S, and the sort's pairs: key (label << bits) | caller, value = the leaf.
// The entries beyond the leaf count get the key 1 << 2 bits, above every real one.
__global__ __launch_bounds__(GTB) void k_groups_keys(int64_t n, const double *__restrict__ leaves,
                                                     const uint32_t *__restrict__ d_count,
                                                     const uint32_t *__restrict__ cidx,
                                                     const uint32_t *__restrict__ rootof,
                                                     const uint32_t *__restrict__ minc, int bits,
                                                     int64_t *__restrict__ label,
                                                     uint64_t *__restrict__ key,
                                                     uint32_t *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i >= n) return;
    val[i] = (uint32_t)i;
    if (i >= (int64_t)*d_count) {
        key[i] = (uint64_t)1 << (2 * bits);
        return;
    }
    const uint32_t slot = (uint32_t)__double_as_longlong(leaves[4 * (size_t)i + 3]);
    const uint32_t c = cidx[slot];
    const uint32_t lab = minc[rootof[i]];
    label[c] = (int64_t)lab;
    key[i] = ((uint64_t)lab << bits) | c;
}

// Over the sorted keys: flag[i] = 1 where a group's run begins (flag has n + 1 entries, the last
// 0, for the scan's total), and members[i] = the caller index.
__global__ __launch_bounds__(GTB) void k_groups_heads(
    int64_t n, const uint64_t *__restrict__ key_s, const uint32_t *__restrict__ d_count, int bits,
    uint32_t *__restrict__ flag, int64_t *__restrict__ members) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i > n) return;
    const bool in = i < (int64_t)*d_count;
    bool head = false;
    if (in) {
        const uint64_t k = key_s[i];
        head = i == 0 || (key_s[i - 1] >> bits) != (k >> bits);
        members[i] = (int64_t)(k & (((uint64_t)1 << bits) - 1));
    }
    flag[i] = head ? 1u : 0u;
}

// first[g] = where run g begins, first[number of runs] = the leaf count (gid: the exclusive
// scan of flag, gid[n] = the number of runs).
__global__ __launch_bounds__(GTB) void k_groups_first(int64_t n, const uint32_t *__restrict__ flag,
                                                      const uint32_t *__restrict__ gid,
                                                      const uint32_t *__restrict__ d_count,
                                                      uint32_t *__restrict__ first) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) first[gid[i]] = (uint32_t)i;
    if (i == 0) first[gid[n]] = *d_count;
}

// keep[g] = 1 iff run g has at least min_members members (n + 1 entries, the last 0).
__global__ __launch_bounds__(GTB) void k_groups_keep(int64_t n, const uint32_t *__restrict__ gid,
                                                     const uint32_t *__restrict__ first,
                                                     int64_t min_members,
                                                     uint32_t *__restrict__ keep) {
    const int64_t g = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (g > n) return;
    const bool is = g < (int64_t)gid[n];
    keep[g] = is && (int64_t)(first[g + 1] - first[g]) >= min_members ? 1u : 0u;
}

// The slot of the partials of block k of run g, which begins at f: injective over all blocks of
// all runs, below groups_partial_slots(n).
__device__ __forceinline__ size_t partial_slot(uint32_t f, uint32_t g, uint32_t k) {
    return (size_t)(f / GRP_BLOCK) + g + k;
}

// One lane per 256-member block of a kept group: the sequential sums of its members' terms in
// ascending caller index, from +0.0.  part: five planes of `slots` entries.
__global__ __launch_bounds__(GTB) void k_groups_partials(
    int64_t n, const uint32_t *__restrict__ d_count, const uint32_t *__restrict__ flag,
    const uint32_t *__restrict__ gid, const uint32_t *__restrict__ first,
    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ val_s,
    const double *__restrict__ leaves, const double *__restrict__ vx,
    const double *__restrict__ vy, double *__restrict__ part, size_t slots) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i >= n || i >= (int64_t)*d_count) return;
    const uint32_t g = gid[i] - (flag[i] ? 0u : 1u);
    if (!keep[g]) return;
    const uint32_t f = first[g], rel = (uint32_t)i - f;
    if (rel % GRP_BLOCK) return;
    const uint32_t end = min((uint32_t)i + GRP_BLOCK, first[g + 1]);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (uint32_t j = (uint32_t)i; j < end; ++j) {
        const double4_t r = reinterpret_cast<const double4_t *>(leaves)[val_s[j]];
        const uint32_t slot = (uint32_t)__double_as_longlong(r.w);
        const double m = r.z;
        s0 = s0 + m;
        s1 = s1 + m * r.x;
        s2 = s2 + m * r.y;
        s3 = s3 + m * vx[slot];
        s4 = s4 + m * vy[slot];
    }
    const size_t at = partial_slot(f, g, rel / GRP_BLOCK);
    part[at] = s0;
    part[slots + at] = s1;
    part[2 * slots + at] = s2;
    part[3 * slots + at] = s3;
    part[4 * slots + at] = s4;
}

// One lane per kept group: its record, the sums over its blocks' partials in order from +0.0.
__global__ __launch_bounds__(GTB) void k_groups_emit(
    int64_t n, const uint32_t *__restrict__ gid, const uint32_t *__restrict__ first,
    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kidx,
    const uint64_t *__restrict__ key_s, int bits, const double *__restrict__ part, size_t slots,
    bh_group *__restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (g >= n || g >= (int64_t)gid[n] || !keep[g]) return;
    const uint32_t f = first[g], cnt = first[g + 1] - f;
    const uint32_t nb = (cnt + GRP_BLOCK - 1) / GRP_BLOCK;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = 0; k < nb; ++k) {
        const size_t at = partial_slot(f, (uint32_t)g, k);
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] = s[q] + part[q * slots + at];
    }
    bh_group r;
    r.label = (int64_t)(key_s[f] >> bits);
    r.count = (int64_t)cnt;
    r.first = (int64_t)f;
    r.mass = s[0];
    r.mx = s[1];
    r.my = s[2];
    r.px = s[3];
    r.py = s[4];
    out[kidx[g]] = r;
}

// The summary, by one workgroup: the largest group under (count, lower label) by a strided pass
// and a tree reduction in a fixed order -- an integer maximum.  sum: the six fields of
// bh_groups_summary; with S empty all 0 but largest_label = -1.
__global__ __launch_bounds__(SUM_TB) void k_groups_summary(
    int64_t n, const uint32_t *__restrict__ d_count, const uint32_t *__restrict__ gid,
    const uint32_t *__restrict__ first, const uint32_t *__restrict__ kidx,
    const uint64_t *__restrict__ key_s, int bits, int64_t *__restrict__ sum) {
    __shared__ uint64_t best[SUM_TB];
    const uint32_t G = gid[n];
    uint64_t mine = 0;  // (count << 32) | (0xFFFFFFFF - label): the maximum is the largest
    for (uint32_t g = threadIdx.x; g < G; g += SUM_TB) {
        const uint32_t f = first[g], cnt = first[g + 1] - f;
        const uint32_t lab = (uint32_t)(key_s[f] >> bits);
        const uint64_t k = ((uint64_t)cnt << 32) | (0xFFFFFFFFu - lab);
        mine = k > mine ? k : mine;
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int w = SUM_TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const uint64_t o = best[threadIdx.x + w];
            if (o > best[threadIdx.x]) best[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const uint32_t nl = *d_count;
    sum[0] = nl ? n : 0;
    sum[1] = (int64_t)nl;
    sum[2] = (int64_t)G;
    sum[3] = (int64_t)kidx[n];
    sum[4] = nl ? (int64_t)(0xFFFFFFFFu - (uint32_t)best[0]) : -1;
    sum[5] = (int64_t)(best[0] >> 32);
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + GTB - 1) / GTB); }

int key_bits(int64_t n) {  // caller indices and labels are below the list's size
    int bits = 1;
    while (((int64_t)1 << bits) < n) ++bits;
    return bits;
}

}  // namespace

size_t groups_partial_slots(int64_t n) { return (size_t)n / GRP_BLOCK + (size_t)n + 2; }

size_t groups_scratch_bytes(int64_t n) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u,
                                    (unsigned)(2 * key_bits(n) + 1));
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u,
                                  (size_t)(n + 1), rocprim::plus<uint32_t>());
    return a > b ? a : b;
}

void groups_prepare(int64_t n, const GroupBufs &B, hipStream_t s) {
    if (n <= 0) return;
    k_groups_init<<<blocks(n), GTB, 0, s>>>(n, B.parent, B.minc, B.label);
}

hipError_t groups_run(const Node *nodes, size_t node_cap, const uint32_t *d_T,
                      const uint32_t *cidx, const LeafList &leaves, const uint32_t *d_count,
                      const double *vx, const double *vy, int64_t n, double link,
                      int64_t min_members, const NeighborReach &rc, const GroupBufs &B,
                      hipStream_t s) {
    if (n <= 0) return hipSuccess;
    {  // the link walk, in the launch shape the other walks choose for n lanes
        const WalkShape w = walk_shape(n);
        if (node_off32(node_cap))
            k_groups_link<true><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, leaves.rec, d_count,
                                                              link, rc, B.parent, w.bpw, w.wpb);
        else
            k_groups_link<false><<<w.grid, TB * w.wpb, 0, s>>>(nodes, d_T, leaves.rec, d_count,
                                                               link, rc, B.parent, w.bpw, w.wpb);
    }
    const int bits = key_bits(n);
    const size_t slots = groups_partial_slots(n);
    k_groups_root<<<blocks(n), GTB, 0, s>>>(leaves.rec, d_count, cidx, B.parent, B.rootof, B.minc);
    k_groups_keys<<<blocks(n), GTB, 0, s>>>(n, leaves.rec, d_count, cidx, B.rootof, B.minc, bits,
                                            B.label, B.key, B.val);
    size_t bytes = B.scratch_bytes;
    hipError_t st = rocprim::radix_sort_pairs(B.scratch, bytes, B.key, B.key_s, B.val, B.val_s,
                                              (size_t)n, 0u, (unsigned)(2 * bits + 1), s);
    if (st != hipSuccess) return st;
    k_groups_heads<<<blocks(n + 1), GTB, 0, s>>>(n, B.key_s, d_count, bits, B.flag, B.members);
    bytes = B.scratch_bytes;
    st = rocprim::exclusive_scan(B.scratch, bytes, B.flag, B.gid, 0u, (size_t)(n + 1),
                                 rocprim::plus<uint32_t>(), s);
    if (st != hipSuccess) return st;
    k_groups_first<<<blocks(n), GTB, 0, s>>>(n, B.flag, B.gid, d_count, B.first);
    k_groups_keep<<<blocks(n + 1), GTB, 0, s>>>(n, B.gid, B.first, min_members, B.keep);
    bytes = B.scratch_bytes;
    st = rocprim::exclusive_scan(B.scratch, bytes, B.keep, B.kidx, 0u, (size_t)(n + 1),
                                 rocprim::plus<uint32_t>(), s);
    if (st != hipSuccess) return st;
    k_groups_partials<<<blocks(n), GTB, 0, s>>>(n, d_count, B.flag, B.gid, B.first, B.keep, B.val_s,
                                                leaves.rec, vx, vy, B.part, slots);
    k_groups_emit<<<blocks(n), GTB, 0, s>>>(n, B.gid, B.first, B.keep, B.kidx, B.key_s, bits,
                                            B.part, slots, B.groups);
    k_groups_summary<<<1, SUM_TB, 0, s>>>(n, d_count, B.gid, B.first, B.kidx, B.key_s, bits,
                                          B.summary);
    return hipGetLastError();
}

}  // namespace bh
