// The bodies in annuli about a centre (bh_compute_radial_profile, include/bh_engine.h;
// DESIGN.md §21).
//
// The planes x, y, vx, vy, m arrive in the caller's list order, so lane i is caller index i.
// The terms of body c, in binary64, every operation separate (the build never contracts):
//     dx = x - cx;  dy = y - cy;  R2 = dx*dx + dy*dy;  R = sqrt(R2)
//     ux = vx - cvx;  uy = vy - cvy;  u = dx*ux + dy*uy;  w = dx*uy - dy*ux
//     vr = u / R;  vt = w / R;  R2 == 0.0: vr = vt = +0.0
//     m, m*R, m*vr, m*vt, (m*vr)*vr, (m*vt)*vt, m*w
// Body c is in bin k iff edges[k] <= R && R < edges[k+1].
//
// The chain: a key per caller index -- its bin, or one of four class keys above the bins (inner,
// outer, NaN, not selected) -- from a binary search of R in the edges held in LDS; one stable
// radix sort of (key, caller index) over the bits n_bin + 4 keys need, which leaves every bin's
// members in ascending caller index; where each key begins, by a lower bound per key (the class
// counts of the summary are differences of these, so no counter and no atomic of any kind is
// needed); the seven terms by sorted position into seven contiguous planes; then bh_group's two
// fixed-order levels with the bin as the label: one lane per (256-member block, term) sums its
// block from +0.0, one lane per (bin, term) sums the bin's block partials from +0.0.
#include <rocprim/device/device_radix_sort.hpp>

#include "bh_device.hpp"

namespace bh {
namespace {

constexpr int RTB = 256;
constexpr uint32_t RAD_BLOCK = 256;  // members per block of a bin's two-level sums
constexpr int RAD_TERMS = 7;
constexpr unsigned KEY_GRID_MAX = 2048;  // the keys kernel strides: each workgroup stages the edges

__device__ __forceinline__ double radial_R(double x, double y, double cx, double cy, double &dx,
                                           double &dy, double &R2) {
    dx = x - cx;
    dy = y - cy;
    R2 = dx * dx + dy * dy;
    return sqrt(R2);
}

// flag[c] = 1 for every caller index of the subset: plain stores of one value, so lanes that
// meet on a duplicate do no harm.
__global__ __launch_bounds__(RTB) void k_radial_mark(int64_t n, const int64_t *__restrict__ subset,
                                                     int64_t n_subset,
                                                     uint8_t *__restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * RTB + threadIdx.x;
    if (j >= n_subset) return;
    const int64_t c = subset[j];
    if (c >= 0 && c < n) flag[c] = 1;  // (the host refused every other index)
}

// key[i]: the bin of caller index i, or n_bin + class.  The number of edges <= R, found without
// a branch on the data, is the bin + 1; 0 of them: inner; all n_bin + 1: outer.
__global__ __launch_bounds__(RTB) void k_radial_keys(
    int64_t n, const double *__restrict__ x, const double *__restrict__ y, double cx, double cy,
    uint32_t n_bin, const double *__restrict__ edges, const uint8_t *__restrict__ flag,
    uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    extern __shared__ double s_edges[];
    for (uint32_t j = threadIdx.x; j <= n_bin; j += RTB) s_edges[j] = edges[j];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * RTB + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * RTB) {
        double dx, dy, R2;
        const double R = radial_R(x[i], y[i], cx, cy, dx, dy, R2);
        uint32_t lo = 0, len = n_bin + 1;
        while (len > 0) {
            const uint32_t half = len >> 1;
            const bool le = s_edges[lo + half] <= R;
            lo = le ? lo + half + 1 : lo;
            len = le ? len - half - 1 : half;
        }
        uint32_t k = lo - 1;
        if (lo == 0) k = n_bin + RADIAL_INNER;
        if (lo == n_bin + 1) k = n_bin + RADIAL_OUTER;
        if (R != R) k = n_bin + RADIAL_NAN;
        if (flag && !flag[i]) k = n_bin + RADIAL_UNSELECTED;
        key[i] = k;
        val[i] = (uint32_t)i;
    }
}

// start[k], k <= n_bin + 4: the first sorted position whose key is >= k (start[n_bin + 4] = n).
__global__ __launch_bounds__(RTB) void k_radial_starts(int64_t n, uint32_t n_bin,
                                                       const uint32_t *__restrict__ key_s,
                                                       uint32_t *__restrict__ start) {
    const uint32_t k = blockIdx.x * RTB + threadIdx.x;
    if (k > n_bin + 4) return;
    uint32_t lo = 0, hi = (uint32_t)n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key_s[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    start[k] = lo;
}

// The seven terms of the body at sorted position i, for the positions that lie in a bin.
__global__ __launch_bounds__(RTB) void k_radial_terms(
    int64_t n, const double *__restrict__ x, const double *__restrict__ y,
    const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ m,
    double cx, double cy, double cvx, double cvy, uint32_t n_bin,
    const uint32_t *__restrict__ start, const uint32_t *__restrict__ val_s,
    double *__restrict__ terms) {
    const int64_t i = (int64_t)blockIdx.x * RTB + threadIdx.x;
    if (i >= n || i >= (int64_t)start[n_bin]) return;
    const uint32_t c = val_s[i];
    double dx, dy, R2;
    const double R = radial_R(x[c], y[c], cx, cy, dx, dy, R2);
    const double ux = vx[c] - cvx, uy = vy[c] - cvy;
    const double u = dx * ux + dy * uy;
    const double w = dx * uy - dy * ux;
    double vr = u / R, vt = w / R;
    if (R2 == 0.0) vr = vt = 0.0;
    const double mc = m[c];
    const double mvr = mc * vr, mvt = mc * vt;
    const size_t N = (size_t)n;
    terms[i] = mc;
    terms[N + i] = mc * R;
    terms[2 * N + i] = mvr;
    terms[3 * N + i] = mvt;
    terms[4 * N + i] = mvr * vr;
    terms[5 * N + i] = mvt * vt;
    terms[6 * N + i] = mc * w;
}

// The slot of the partials of block k of bin b, which begins at f: injective over all blocks of
// all bins (a later bin begins at or after f + count and has a higher b), below
// radial_partial_slots(n).
__device__ __forceinline__ size_t partial_slot(uint32_t f, uint32_t b, uint32_t k) {
    return (size_t)(f / RAD_BLOCK) + b + k;
}

// One lane per (256-member block of a bin, term): the sequential sum of the block's terms in
// ascending caller index, from +0.0.  blockIdx.y: the term.
__global__ __launch_bounds__(RTB) void k_radial_partials(
    int64_t n, uint32_t n_bin, const uint32_t *__restrict__ start,
    const uint32_t *__restrict__ key_s, const double *__restrict__ terms,
    double *__restrict__ part, size_t slots) {
    const int64_t i = (int64_t)blockIdx.x * RTB + threadIdx.x;
    if (i >= n || i >= (int64_t)start[n_bin]) return;
    const uint32_t b = key_s[i];
    const uint32_t f = start[b], rel = (uint32_t)i - f;
    if (rel % RAD_BLOCK) return;
    const uint32_t end = min((uint32_t)i + RAD_BLOCK, start[b + 1]);
    const double *t = terms + (size_t)blockIdx.y * (size_t)n;
    double s = 0.0;
#pragma unroll 8
    for (uint32_t j = (uint32_t)i; j < end; ++j) s = s + t[j];
    part[(size_t)blockIdx.y * slots + partial_slot(f, b, rel / RAD_BLOCK)] = s;
}

// One lane per (bin, term): the sequential sum of the bin's block partials in order from +0.0
// into the record's field of that term; the lane of term 0 writes the count too.
__global__ __launch_bounds__(RTB) void k_radial_emit(uint32_t n_bin,
                                                     const uint32_t *__restrict__ start,
                                                     const double *__restrict__ part, size_t slots,
                                                     bh_radial_bin *__restrict__ out) {
    const uint32_t b = blockIdx.x * RTB + threadIdx.x;
    if (b >= n_bin) return;
    const uint32_t f = start[b], cnt = start[b + 1] - f;
    const uint32_t nb = (cnt + RAD_BLOCK - 1) / RAD_BLOCK;
    const double *p = part + (size_t)blockIdx.y * slots + partial_slot(f, b, 0);
    double s = 0.0;
#pragma unroll 8
    for (uint32_t k = 0; k < nb; ++k) s = s + p[k];
    static_assert(sizeof(bh_radial_bin) == 8 * (1 + RAD_TERMS), "count, then the seven sums");
    reinterpret_cast<double *>(out + b)[1 + blockIdx.y] = s;
    if (blockIdx.y == 0) out[b].count = (int64_t)cnt;
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + RTB - 1) / RTB); }

int key_bits(int32_t n_bin) {  // the keys are below n_bin + 4
    int bits = 1;
    while ((1 << bits) < n_bin + 4) ++bits;
    return bits;
}

}  // namespace

size_t radial_partial_slots(int64_t n) {
    return (size_t)n / RAD_BLOCK + (size_t)BH_RADIAL_MAX_BINS + 2;
}

size_t radial_scratch_bytes(int64_t n) {  // the most any bin count asks for
    size_t most = 0;
    for (int bits = 1; bits <= key_bits(BH_RADIAL_MAX_BINS); ++bits) {
        size_t a = 0;
        (void)rocprim::radix_sort_pairs(nullptr, a, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                        (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n,
                                        0u, (unsigned)bits);
        most = a > most ? a : most;
    }
    return most;
}

hipError_t radial_run(int64_t n, const double *x, const double *y, const double *vx,
                      const double *vy, const double *m, double cx, double cy, double cvx,
                      double cvy, int32_t n_bin, bool selected, const int64_t *subset,
                      int64_t n_subset, bool want_bins, const RadialBufs &B, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (selected) {
        hipError_t st = hipMemsetAsync(B.flag, 0, (size_t)n, s);
        if (st != hipSuccess) return st;
        if (n_subset > 0)
            k_radial_mark<<<blocks(n_subset), RTB, 0, s>>>(n, subset, n_subset, B.flag);
    }
    const unsigned kgrid = blocks(n) < KEY_GRID_MAX ? blocks(n) : KEY_GRID_MAX;
    k_radial_keys<<<kgrid, RTB, sizeof(double) * ((size_t)n_bin + 1), s>>>(
        n, x, y, cx, cy, (uint32_t)n_bin, B.edges, selected ? B.flag : nullptr, B.key, B.val);
    size_t bytes = B.scratch_bytes;
    hipError_t st = rocprim::radix_sort_pairs(B.scratch, bytes, B.key, B.key_s, B.val, B.val_s,
                                              (size_t)n, 0u, (unsigned)key_bits(n_bin), s);
    if (st != hipSuccess) return st;
    k_radial_starts<<<blocks(n_bin + 5), RTB, 0, s>>>(n, (uint32_t)n_bin, B.key_s, B.start);
    if (want_bins) {
        const size_t slots = radial_partial_slots(n);
        k_radial_terms<<<blocks(n), RTB, 0, s>>>(n, x, y, vx, vy, m, cx, cy, cvx, cvy,
                                                 (uint32_t)n_bin, B.start, B.val_s, B.terms);
        k_radial_partials<<<dim3(blocks(n), RAD_TERMS), RTB, 0, s>>>(n, (uint32_t)n_bin, B.start,
                                                                     B.key_s, B.terms, B.part, slots);
        k_radial_emit<<<dim3(blocks(n_bin), RAD_TERMS), RTB, 0, s>>>((uint32_t)n_bin, B.start,
                                                                     B.part, slots, B.bins);
    }
    return hipGetLastError();
}

}  // namespace bh
