// All-pairs sum over the leaf sequence for an arbitrary list of targets (bh_compute_field_direct,
// bh_compute_force_error; include/bh_engine.h).
//
// The sequence is direct.hip's: the non-empty leaves of the last tree in pre-order, massless
// subtrees left out (leaf_list_build), one record (x, y, m, slot) per leaf.  A target is either
//   a probe -- a Body(tx, ty, 0, 0, tm) that is not in the tree: no leaf is skipped, a probe that
//     sits on a body gets that body's full term (field.hip's walk with every node opened), or
//   a body  -- a body of the state with its slot: its own leaf is skipped by identity (BHA:219);
//     a body outside the root cell has no leaf and is summed like a probe of its own mass.
// Every leaf, in sequence order, adds
//     dx = lx - tx;  dy = ly - ty;  r2 = dx*dx + dy*dy + soft2
//     invR = 1.0 / sqrt(r2);  invR2 = 1.0 / r2;  f = (G * tm) * lm * invR2          (BHA:250-259)
//     fx += f * dx * invR;  fy += f * dy * invR;  s += lm * invR                     (from +0.0)
// and a = F / tm (BHA:390-391), phi = -(G * s): the additions of the theta = 0 walk in its own
// order, so the bits are the walk's (probes: k_field, bodies: k_direct / the force walk).
//
// The sum of one target is sequential by contract, so the sources cannot be split: the only
// parallelism is across targets.  Two launch shapes (direct_field_shape): up to SMALL_MAX targets
// every workgroup is ONE wave with one target per lane and a 256-leaf tile of its own, so that a
// few thousand targets spread over as many CUs as they have waves; above it k_direct's shape,
// 256 lanes with two targets per lane around a 1024-leaf tile.  Either way a lane stages
// TILE / LANES = 4 records per tile, fetched into registers while the previous tile is summed.
#include "bh_device.hpp"
#include "fastmath.hpp"

namespace bh {
namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int TB = 256;
constexpr int U = 4;  // leaf records read from LDS together (direct.hip BH_DIRECT_U)

#ifndef BH_DFIELD_SMALL_MAX
// Targets up to which the one-wave shape is launched.  Measured on the C5 tree with each shape
// alone (profiles/direct_field_timing.jsonl): the one-wave shape takes 26.5-27.6 ms
// up to 32 768 targets against 41.9-42.1 ms for the other, and 43.6 against 42.2 ms at 65 536.
#define BH_DFIELD_SMALL_MAX 32768
#endif

// FAST: every lane of the wave satisfies lane_fast_ok (fastmath.hpp): the seeded sequences equal
// the IEEE operations for every r2 of the sum.  A body's own leaf is then not branched around in
// the force (its dx = dy = +0.0 make the term an exact +-0 with f finite, lane_self_ok), exactly
// as direct.hip's leaf_terms argues; its potential term is not zero and is always selected out.
// A probe excuses nothing on either path.
template <bool FAST, bool BODY, int NBT>
__device__ __forceinline__ void target_terms(const double4_t &r, const double (&tx)[NBT],
                                             const double (&ty)[NBT], const double (&Gm)[NBT],
                                             double soft2, const uint32_t (&self)[NBT],
                                             double (&fx)[NBT], double (&fy)[NBT],
                                             double (&s)[NBT]) {
#pragma unroll
    for (int b = 0; b < NBT; ++b) {
        const double dx = r.x - tx[b];  // BHA:251-253
        const double dy = r.y - ty[b];
        const double r2 = dx * dx + dy * dy + soft2;
        const bool other = !BODY || (uint32_t)__double_as_longlong(r.w) != self[b];  // BHA:219
        if (FAST) {
            double h;
            const double rr = sqrt_rn_inrange_h(r2, h);
            const double invR = rcp_rn_seeded(rr, h + h);
            const double invR2 = rcp_rn_seeded(r2, invR * invR);
            const double f = Gm[b] * r.z * invR2;
            fx[b] += f * dx * invR;
            fy[b] += f * dy * invR;
            s[b] += other ? r.z * invR : 0.0;  // (s is from +0.0 and never -0.0: + 0.0 keeps it)
        } else if (other) {
            const double invR = 1.0 / sqrt(r2);
            const double invR2 = 1.0 / r2;
            const double f = Gm[b] * r.z * invR2;
            fx[b] += f * dx * invR;
            fy[b] += f * dy * invR;
            s[b] += r.z * invR;
        }
    }
}

template <bool FAST, bool BODY, int NBT>
__device__ __forceinline__ void sum_tile(const double4_t *s_rec, int cnt, const double (&tx)[NBT],
                                         const double (&ty)[NBT], const double (&Gm)[NBT],
                                         double soft2, const uint32_t (&self)[NBT],
                                         double (&fx)[NBT], double (&fy)[NBT], double (&s)[NBT]) {
    int j = 0;
    for (; j + U <= cnt; j += U) {
        double4_t r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = s_rec[j + u];  // broadcast reads, issued together
#pragma unroll
        for (int u = 0; u < U; ++u)
            target_terms<FAST, BODY, NBT>(r[u], tx, ty, Gm, soft2, self, fx, fy, s);
    }
    for (; j < cnt; ++j) target_terms<FAST, BODY, NBT>(s_rec[j], tx, ty, Gm, soft2, self, fx, fy, s);
}

// Target p = (block * NBT + b) * LANES + lane.  d_count null: no tree (no bodies), L is not read.
// tm null: every target has mass 1.0.  BODY: tslot[p] is the target's body slot, and phi is not
// written (the force error wants accelerations alone; the dead sum is dropped by the compiler).
template <bool BODY, int LANES, int NBT, int TILE>
__global__ __launch_bounds__(LANES) void k_direct_targets(LeafList L,
                                                          const uint32_t *__restrict__ d_count,
                                                          const double *__restrict__ tx_,
                                                          const double *__restrict__ ty_,
                                                          const double *__restrict__ tm_,
                                                          const uint32_t *__restrict__ tslot,
                                                          int64_t n, double G, double soft2,
                                                          double *__restrict__ ax,
                                                          double *__restrict__ ay,
                                                          double *__restrict__ phi) {
    static_assert(TILE % LANES == 0 && TILE % U == 0, "whole staging passes, whole unrolls");
    constexpr int PER = TILE / LANES;  // records a lane stages per tile
    __shared__ double4_t s_rec[TILE];
    int64_t p[NBT];
    bool valid[NBT];
    double tx[NBT], ty[NBT], tm[NBT], Gm[NBT], fx[NBT], fy[NBT], s[NBT];
    uint32_t self[NBT];
    bool slow = false;
#pragma unroll
    for (int b = 0; b < NBT; ++b) {
        p[b] = ((int64_t)blockIdx.x * NBT + b) * LANES + threadIdx.x;
        valid[b] = p[b] < n;
        tx[b] = valid[b] ? tx_[p[b]] : 0.0;
        ty[b] = valid[b] ? ty_[p[b]] : 0.0;
        tm[b] = valid[b] && tm_ ? tm_[p[b]] : 1.0;
        Gm[b] = G * tm[b];  // (Config.G * b.m) first (BHA:256)
        self[b] = BODY && valid[b] ? tslot[p[b]] : 0xFFFFFFFFu;
        bool ok = lane_fast_ok(tx[b], ty[b], soft2);
        if (BODY) ok = ok && lane_self_ok(Gm[b], tm[b]);
        slow |= valid[b] && !ok;
        fx[b] = 0.0;
        fy[b] = 0.0;
        s[b] = 0.0;
    }
    const bool fast = __ballot(slow) == 0ull;  // per wave
    const uint32_t nl = d_count ? *d_count : 0u;
    const double4_t *rec = reinterpret_cast<const double4_t *>(L.rec);
    double4_t nxt[PER];
    auto fetch = [&](uint32_t t0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t i = t0 + k * LANES + threadIdx.x;  // (nl <= 2^30: no wrap)
            nxt[k] = i < nl ? rec[i] : double4_t{0.0, 0.0, 0.0, 0.0};  // (past cnt: never read)
        }
    };
    fetch(0);
    for (uint32_t t0 = 0; t0 < nl; t0 += TILE) {
        const int cnt = (int)min((uint32_t)TILE, nl - t0);
        __syncthreads();  // the previous tile's readers are done
#pragma unroll
        for (int k = 0; k < PER; ++k) s_rec[k * LANES + threadIdx.x] = nxt[k];
        __syncthreads();
        if (t0 + TILE < nl) fetch(t0 + TILE);  // in flight while this tile is summed
        if (fast)
            sum_tile<true, BODY, NBT>(s_rec, cnt, tx, ty, Gm, soft2, self, fx, fy, s);
        else
            sum_tile<false, BODY, NBT>(s_rec, cnt, tx, ty, Gm, soft2, self, fx, fy, s);
    }
#pragma unroll
    for (int b = 0; b < NBT; ++b) {
        if (!valid[b]) continue;
        ax[p[b]] = fx[b] / tm[b];  // BHA:390-391
        ay[p[b]] = fy[b] / tm[b];
        if (!BODY) phi[p[b]] = -(G * s[b]);
    }
}

// slot_of[caller index] = slot (tombstones have none; slot_of is 0xFF-filled before)
__global__ __launch_bounds__(TB) void k_slot_of(int64_t n, const uint32_t *__restrict__ cidx,
                                                uint32_t *__restrict__ slot_of) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cidx[i];
    if (!(c & CIDX_DEAD) && (int64_t)c < n) slot_of[c] = (uint32_t)i;
}

// Sample j = the body at caller index idx[j] (validated by the host: < n): its position, mass and
// slot as the build left them, and its acceleration of the evaluation just made (caller order).
__global__ __launch_bounds__(TB) void k_body_targets(int64_t k, const uint32_t *__restrict__ idx,
                                                     const uint32_t *__restrict__ slot_of,
                                                     int64_t n, BodyState st,
                                                     const double *__restrict__ ax_c,
                                                     const double *__restrict__ ay_c,
                                                     double *__restrict__ tx,
                                                     double *__restrict__ ty,
                                                     double *__restrict__ tm,
                                                     uint32_t *__restrict__ tslot,
                                                     double *__restrict__ ax_tree,
                                                     double *__restrict__ ay_tree) {
    const int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (j >= k) return;
    const uint32_t c = idx[j];
    const double nan = __builtin_nan("");
    if ((int64_t)c >= n) {  // (never: the host validated idx against this list)
        tx[j] = ty[j] = tm[j] = ax_tree[j] = ay_tree[j] = nan;
        tslot[j] = 0xFFFFFFFFu;
        return;
    }
    const uint32_t sl = slot_of[c];
    const bool have = (int64_t)sl < n;  // (always, between calls: every caller index is live)
    tx[j] = have ? st.x[sl] : nan;
    ty[j] = have ? st.y[sl] : nan;
    tm[j] = have ? st.m[sl] : nan;
    tslot[j] = sl;
    ax_tree[j] = ax_c[c];
    ay_tree[j] = ay_c[c];
}

template <bool BODY>
void launch_targets(const DirectFieldShape &sh, const LeafList &L, const uint32_t *d_count,
                    const double *tx, const double *ty, const double *tm, const uint32_t *tslot,
                    int64_t n, double G, double soft2, double *ax, double *ay, double *phi,
                    hipStream_t s) {
    const unsigned grid = (unsigned)((n + sh.lanes * sh.per_lane - 1) / (sh.lanes * sh.per_lane));
    if (sh.lanes == 64)
        k_direct_targets<BODY, 64, 1, 256><<<grid, 64, 0, s>>>(L, d_count, tx, ty, tm, tslot, n, G,
                                                               soft2, ax, ay, phi);
    else
        k_direct_targets<BODY, 256, 2, 1024><<<grid, 256, 0, s>>>(L, d_count, tx, ty, tm, tslot, n,
                                                                  G, soft2, ax, ay, phi);
}

}  // namespace

DirectFieldShape direct_field_shape(int64_t n_target) {
    if (n_target <= (int64_t)BH_DFIELD_SMALL_MAX) return DirectFieldShape{256, 64, 1};
    return DirectFieldShape{1024, 256, 2};
}

void direct_targets(const LeafList &L, const uint32_t *d_count, const double *tx, const double *ty,
                    const double *tm, const uint32_t *tslot, int64_t n, double G, double soft2,
                    double *ax, double *ay, double *phi, hipStream_t s) {
    if (n <= 0) return;
    const DirectFieldShape sh = direct_field_shape(n);
    if (tslot)
        launch_targets<true>(sh, L, d_count, tx, ty, tm, tslot, n, G, soft2, ax, ay, phi, s);
    else
        launch_targets<false>(sh, L, d_count, tx, ty, tm, tslot, n, G, soft2, ax, ay, phi, s);
}

hipError_t direct_body_targets(int64_t n, const BodyState &st, const uint32_t *idx, int64_t k,
                               uint32_t *slot_of, const double *ax_c, const double *ay_c,
                               double *tx, double *ty, double *tm, uint32_t *tslot,
                               double *ax_tree, double *ay_tree, hipStream_t s) {
    if (n <= 0 || k <= 0) return hipSuccess;
    hipError_t rc = hipMemsetAsync(slot_of, 0xFF, sizeof(uint32_t) * (size_t)n, s);
    if (rc != hipSuccess) return rc;
    k_slot_of<<<(unsigned)((n + TB - 1) / TB), TB, 0, s>>>(n, st.cidx, slot_of);
    k_body_targets<<<(unsigned)((k + TB - 1) / TB), TB, 0, s>>>(k, idx, slot_of, n, st, ax_c, ay_c,
                                                                tx, ty, tm, tslot, ax_tree,
                                                                ay_tree);
    return hipGetLastError();
}

}  // namespace bh
