// The k nearest bodies of probe points and of the bodies themselves (bh_find_knn,
// bh_find_knn_bodies, include/bh_engine.h).
//
// The candidate set and the exact test are bh_find_neighbors' (neighbors.hip): body b of the leaf
// sequence is a candidate of probe j iff dx*dx + dy*dy <= r_max*r_max in binary64, nothing fused,
// made on the leaf's node record.  Row j is the first min(k, candidates) of them under the total
// order (d2, caller index).
//
// The walk is neighbor_walk.hpp's, mode NBR_KNN: one lane = one probe, and the lane keeps its k
// best so far in a binary max-heap in LDS (KnnHeap below).  Until the heap is full the lane's
// radius is its seed; from then on it is the heap's root, the k-th best so far, and shrinks with
// every accepted hit -- what NBR_PICK does for k = 1.
//
// The seed (k_knn_seed) is what makes the pre-order walk prune from its first stop: an upper
// bound on the lane's k-th distance, formed from k real members of the candidate set -- windows
// of the leaf sequence at the place a binary search on the build's Morton key gives the probe.  Which window is taken changes the work, never the result: the list starts empty and the
// walk meets the window's leaves again.
//
// Every output is an integer or a d2 that one candidate's arithmetic produced: no floating-point
// sum, no atomic.
#include "bh_device.hpp"
#include "neighbor_walk.hpp"

namespace bh {
namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));  // one leaf record

constexpr uint32_t KNN_LDS_BUDGET = 64u * 1024u;  // per workgroup: two or more fit a CU's 160 KiB
constexpr uint32_t KNN_ENTRY_BYTES = 12;          // d2 (8) + caller index (4)

__device__ __forceinline__ bool knn_less(double ad, uint32_t ac, double bd, uint32_t bc) {
    return ad < bd || (ad == bd && ac < bc);
}

// A lane's list: a binary max-heap under (d2, caller index) of up to k entries, structure of
// arrays and lane-strided -- entry i of the lane at d[i * 64] and c[i * 64], so that the 64 lanes
// of a wave touch 64 consecutive words when they touch the same entry.  Only the lane itself ever
// reads or writes its column: no barrier anywhere.  The number of entries is the lane's L.found
// (the walk takes its functor by value; what changes lives in the lane).
struct KnnHeap {
    double *d;
    uint32_t *c;
    uint32_t k;
    uint32_t self;  // bh_find_knn_bodies: the lane's own body slot, never a hit (else no slot)

    // (vd, vc) into the hole at the root of the first m entries, moving larger children up
    __device__ __forceinline__ void sift_down(uint32_t m, double vd, uint32_t vc) const {
        uint32_t i = 0;
        for (;;) {
            uint32_t ch = 2 * i + 1;
            if (ch >= m) break;
            double cd = d[ch * 64];
            uint32_t cc = c[ch * 64];
            if (ch + 1 < m) {
                const double rd = d[(ch + 1) * 64];
                const uint32_t rc = c[(ch + 1) * 64];
                if (knn_less(cd, cc, rd, rc)) {
                    cd = rd;
                    cc = rc;
                    ++ch;
                }
            }
            if (!knn_less(vd, vc, cd, cc)) break;
            d[i * 64] = cd;
            c[i * 64] = cc;
            i = ch;
        }
        d[i * 64] = vd;
        c[i * 64] = vc;
    }

    // the lane's radius becomes the k-th best so far (correctly rounded sqrt; the pad covers it)
    __device__ __forceinline__ void shrink(NbrLane &L) const {
        const double worst = d[0];
        L.r2 = worst;
        L.rp = __builtin_sqrt(worst) * NEIGHBOR_RADIUS_PAD;
    }

    // a hit (d2 <= L.r2) of caller index ci
    __device__ __forceinline__ void insert(NbrLane &L, double d2, uint32_t ci) const {
        if (L.found < k) {
            uint32_t i = L.found++;
            while (i > 0) {
                const uint32_t p = (i - 1) >> 1;
                const double pd = d[p * 64];
                const uint32_t pc = c[p * 64];
                if (!knn_less(pd, pc, d2, ci)) break;
                d[i * 64] = pd;
                c[i * 64] = pc;
                i = p;
            }
            d[i * 64] = d2;
            c[i * 64] = ci;
            if (L.found == k) shrink(L);
        } else if (knn_less(d2, ci, d[0], c[0])) {  // replaces the worst
            sift_down(k, d2, ci);
            shrink(L);
        }
    }

    // heap sort in place: entries [0, cnt) ascending under (d2, caller index)
    __device__ __forceinline__ void sort(uint32_t cnt) const {
        for (uint32_t m = cnt; m > 1; --m) {
            const double ld = d[(m - 1) * 64];
            const uint32_t lc = c[(m - 1) * 64];
            d[(m - 1) * 64] = d[0];
            c[(m - 1) * 64] = c[0];
            sift_down(m - 1, ld, lc);
        }
    }
};

// Lane q's probe.  SELF: the body in slot q, whose row is its caller index map[q] = cidx[q] (a
// tombstone has none); else the probe map[q] = order[q] of the caller's list.
template <bool SELF>
__device__ __forceinline__ bool knn_probe(int64_t q, int64_t n, const uint32_t *__restrict__ map,
                                          const double *__restrict__ px,
                                          const double *__restrict__ py, int64_t &row, double &bx,
                                          double &by) {
    row = 0;
    bx = by = 0.0;
    if (q >= n) return false;
    const uint32_t m = map[q];
    if (SELF && (m & CIDX_DEAD)) return false;
    row = (int64_t)m;
    const int64_t p = SELF ? q : row;
    bx = px[p];
    by = py[p];
    return true;
}

// seed[q]: the radius^2 lane q starts from.  The leaf sequence is in pre-order, which is the order
// of the build's Morton keys, so the lower bound of the probe's key is the place of the leaves
// that share the longest key prefix with it.  (Where a jitter left a leaf's key out of order the
// search still ends somewhere in [0, nl]: any window is a valid one.)  A window of W = k
// consecutive leaves near it (SELF: k + 1, the lane's own dropped) gives k members of S; the
// largest of their d2 -- the walk's own expression on the leaf record's x, y, the bits the walk
// meets as that leaf's node record -- bounds the k-th smallest d2 over S from above.  One window
// around the place is not enough: the curve jumps where it leaves a cell, so a window that
// straddles the end of a large cell holds leaves a cell's width away, and one such lane makes its
// whole wave walk that far (C3, k = 8: 24.7 ms with the centred window alone).  The
// window before the place and the window after it lie on one side of such a jump each, so the
// smallest of the three bounds is taken.  With fewer than W leaves, or a cap below it, the seed
// is r_max^2.
constexpr int SEED_TB = 256;
template <bool SELF>
__global__ __launch_bounds__(SEED_TB) void k_knn_seed(const double *__restrict__ leaves,
                                                      const uint32_t *__restrict__ d_count,
                                                      const uint32_t *__restrict__ map,
                                                      const double *__restrict__ px,
                                                      const double *__restrict__ py, int64_t n,
                                                      uint32_t k, double rmax2, Geometry g,
                                                      double *__restrict__ seed) {
    const int64_t q = (int64_t)blockIdx.x * SEED_TB + threadIdx.x;
    if (q >= n) return;
    int64_t row;
    double bx, by;
    const bool valid = knn_probe<SELF>(q, n, map, px, py, row, bx, by);
    const uint32_t nl = d_count ? *d_count : 0u;
    const uint32_t W = SELF ? k + 1 : k;
    double s = rmax2;
    if (valid && bx == bx && by == by && nl >= W) {
        const double4_t *rec = reinterpret_cast<const double4_t *>(leaves);
        const uint64_t key = morton_key(g, bx, by, false);
        uint32_t lo = 0, hi = nl;  // the first leaf whose key is not below the probe's
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const double4_t r = rec[mid];
            if (morton_key(g, r.x, r.y, false) < key)
                lo = mid + 1;
            else
                hi = mid;
        }
        // three windows of W leaves -- the ones before that place, the ones from it on, and the
        // ones around it -- each clipped to the sequence; the smallest of their bounds is taken
        const uint32_t last = nl - W;
        const uint32_t starts[3] = {lo > W ? lo - W : 0u, lo < last ? lo : last,
                                    lo > W / 2 ? (lo - W / 2 < last ? lo - W / 2 : last) : 0u};
        double best = __builtin_inf();
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            double worst = 0.0;
            for (uint32_t i = starts[t]; i < starts[t] + W; ++i) {
                const double4_t r = rec[i];
                if (SELF && (uint32_t)__double_as_longlong(r.w) == (uint32_t)q) continue;
                const double dx = r.x - bx;
                const double dy = r.y - by;
                const double d2 = dx * dx + dy * dy;
                worst = d2 > worst ? d2 : worst;
            }
            best = worst < best ? worst : best;
        }
        const double worst = best;
        s = worst < rmax2 ? worst : rmax2;
    }
    seed[q] = s;
}

// Wave v walks the bpw lanes [bpw v, bpw v + bpw).  The workgroup's LDS holds its waves' heaps:
// the d2 plane of wpb * k * 64 doubles, then the index plane of as many words.  d_T null: no tree
// was built (no bodies).  Row j: idx[j k + i], d2[j k + i] ascending, the tail -1 and +inf;
// found[j] the number of entries.  Each output plane is nullable.
template <bool SELF, bool OFF32>
__global__ __launch_bounds__(TB * MAX_WPB) void k_knn(
    const Node *__restrict__ nodes, const uint32_t *__restrict__ d_T,
    const uint32_t *__restrict__ cidx, const uint32_t *__restrict__ map,
    const double *__restrict__ px, const double *__restrict__ py,
    const double *__restrict__ seed, int64_t n, uint32_t k, NeighborReach rc,
    int64_t *__restrict__ idx, double *__restrict__ d2o, int64_t *__restrict__ found,
    uint32_t bpw, uint32_t wpb) {
    extern __shared__ double knn_lds[];
    const uint32_t v = xcd_run_wave(wpb);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = threadIdx.x >> 6;
    const int64_t q = (int64_t)v * bpw + lane;
    int64_t j;
    NbrLane L;
    const bool valid = knn_probe<SELF>(lane < bpw ? q : n, n, map, px, py, j, L.bx, L.by);
    // a NaN coordinate finds nothing: the lane starts parked, so it never drags the cursor down
    const bool seeks = valid && L.bx == L.bx && L.by == L.by;
    L.r2 = valid ? seed[q] : 0.0;
    L.rp = __builtin_sqrt(L.r2) * NEIGHBOR_RADIUS_PAD;
    L.resume = seeks ? 0u : 0xFFFFFFFFu;
    L.found = 0;
    L.best = __builtin_inf();
    L.bestc = NBR_NONE;
    L.seg = nullptr;
    L.room = 0;
    KnnHeap H;
    H.d = knn_lds + (size_t)w * k * 64 + lane;
    H.c = reinterpret_cast<uint32_t *>(knn_lds + (size_t)wpb * k * 64) + (size_t)w * k * 64 + lane;
    H.k = k;
    H.self = SELF && valid ? (uint32_t)q : NBR_NONE;
    const uint32_t T = d_T ? __builtin_amdgcn_readfirstlane(*d_T) : 0u;
    nbr_walk_wave<NBR_KNN, OFF32>(nodes, T, cidx, rc, L, H);
    if (!valid) return;
    H.sort(L.found);
    const int64_t at = j * (int64_t)k;
    for (uint32_t i = 0; i < k; ++i) {
        const bool in = i < L.found;
        if (idx) idx[at + i] = in ? (int64_t)H.c[i * 64] : (int64_t)-1;
        if (d2o) d2o[at + i] = in ? H.d[i * 64] : __builtin_inf();
    }
    if (found) found[j] = (int64_t)L.found;
}

}  // namespace

KnnShape knn_shape(int64_t lanes, int k) {
    const WalkShape w = walk_shape(lanes);
    KnnShape sh;
    sh.bpw = w.bpw;
    sh.waves = w.waves;
    sh.wpb = w.wpb;
    while (sh.wpb > 1 && sh.wpb * TB * (uint32_t)k * KNN_ENTRY_BYTES > KNN_LDS_BUDGET) sh.wpb >>= 1;
    sh.lds = sh.wpb * TB * (uint32_t)k * KNN_ENTRY_BYTES;
    sh.grid = (sh.waves + sh.wpb - 1) / sh.wpb;
    return sh;
}

void knn_walk(const Node *nodes, size_t node_cap, const uint32_t *d_T, const uint32_t *cidx,
              const LeafList &leaves, const uint32_t *d_count, const uint32_t *map,
              const double *px, const double *py, bool self, int64_t n, int k, double r_max,
              const Geometry &g, const NeighborReach &rc, double *seed, int64_t *idx, double *d2,
              int64_t *found, hipStream_t s) {
    if (n <= 0) return;
    const double rmax2 = r_max * r_max;
    const unsigned sgrid = (unsigned)((n + SEED_TB - 1) / SEED_TB);
    if (self)
        k_knn_seed<true><<<sgrid, SEED_TB, 0, s>>>(leaves.rec, d_count, map, px, py, n, (uint32_t)k,
                                                   rmax2, g, seed);
    else
        k_knn_seed<false><<<sgrid, SEED_TB, 0, s>>>(leaves.rec, d_count, map, px, py, n,
                                                    (uint32_t)k, rmax2, g, seed);
    const KnnShape sh = knn_shape(n, k);
    const bool off32 = node_off32(node_cap);
#define BH_KNN_LAUNCH(S, O)                                                                      \
    k_knn<S, O><<<sh.grid, TB * sh.wpb, sh.lds, s>>>(nodes, d_T, cidx, map, px, py, seed, n,      \
                                                     (uint32_t)k, rc, idx, d2, found, sh.bpw,     \
                                                     sh.wpb)
    if (self) {
        if (off32)
            BH_KNN_LAUNCH(true, true);
        else
            BH_KNN_LAUNCH(true, false);
    } else {
        if (off32)
            BH_KNN_LAUNCH(false, true);
        else
            BH_KNN_LAUNCH(false, false);
    }
#undef BH_KNN_LAUNCH
}

}  // namespace bh
