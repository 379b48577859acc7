// One record of the step log (bh_set_step_log, include/bh_engine.h): the conservation read-out of
// a step, made inside bh_step without a host round trip.
//
// The engine stages the six planes x, y, vx, vy, m, phi of the step's body list L (the state after
// the second kick, before the merge rule) in list order -- mirror_index / mirror_scatter over the
// caller indices, tombstones of the call's earlier steps left out -- and these kernels reduce them
// exactly as diag_reduce (potential.hip) reduces the same list for bh_compute_diagnostics: the
// partition, the per-thread order and the LDS trees are diag_sum.hpp's.  |L| is known only on the
// device once a call has removed bodies, so the kernels read it there (the survivors' count of
// mirror_index) and derive the partition from it: the grid is the largest any n <= n0 can need and
// the workgroups beyond the partition of the actual n leave at once.
#include "bh_device.hpp"
#include "diag_sum.hpp"

namespace bh {
namespace {

// bh_step_record (include/bh_engine.h): int64 step, double t, bh_diagnostics {int64 n, 8 doubles}
constexpr int REC_WORDS = 11;

__device__ __forceinline__ int64_t live_count(int64_t n0, const uint32_t *__restrict__ keep,
                                              const uint32_t *__restrict__ pos) {
    return n0 > 0 ? (int64_t)pos[n0 - 1] + (int64_t)keep[n0 - 1] : 0;
}

__global__ __launch_bounds__(DIAG_TB) void k_log_partial(int64_t n0,
                                                         const uint32_t *__restrict__ keep,
                                                         const uint32_t *__restrict__ pos,
                                                         const double *__restrict__ stage,
                                                         int64_t stride,
                                                         double *__restrict__ part) {
    __shared__ double lds[DIAG_K][DIAG_TB];
    const int64_t n = live_count(n0, keep, pos);
    const DiagPartition dp = diag_partition(n);
    if ((int)blockIdx.x >= dp.blocks) return;  // (uniform over the workgroup)
    diag_partial_block((int)blockIdx.x, n, dp.chunk, stage, stage + stride, stage + 2 * stride,
                       stage + 3 * stride, stage + 4 * stride, stage + 5 * stride, part, lds);
}

// The final sums and the record, by vector stores of one thread.
__global__ __launch_bounds__(DIAG_TB) void k_log_final(int64_t n0,
                                                       const uint32_t *__restrict__ keep,
                                                       const uint32_t *__restrict__ pos,
                                                       const double *__restrict__ part,
                                                       int64_t step, double t,
                                                       unsigned long long *__restrict__ rec) {
    __shared__ double lds[DIAG_K][DIAG_TB];
    const int64_t n = live_count(n0, keep, pos);
    // (n = 0: diagnostics_state returns zeros without a reduction; no partial was written)
    diag_final_block(n > 0 ? diag_partition(n).blocks : 0, part, lds);
    if (threadIdx.x != 0) return;
    rec[0] = (unsigned long long)step;
    rec[1] = (unsigned long long)__double_as_longlong(t);
    rec[2] = (unsigned long long)n;
    for (int k = 0; k < DIAG_K; ++k) {
        const double v = k == 7 ? (n > 0 ? 0.5 * lds[k][0] : 0.0) : lds[k][0];
        rec[3 + k] = (unsigned long long)__double_as_longlong(v);
    }
    static_assert(3 + DIAG_K == REC_WORDS, "bh_step_record is 11 eight-byte words");
}

}  // namespace

void step_log_record(int64_t n0, const uint32_t *keep, const uint32_t *pos, const double *stage,
                     int64_t stride, double *part, int64_t step, double t, void *rec,
                     hipStream_t s) {
    if (n0 > 0) {
        // chunk >= DIAG_TB for every n, so no n <= n0 needs more workgroups than these
        const int64_t most = (n0 + DIAG_TB - 1) / DIAG_TB;
        const int grid = (int)(most < DIAG_MAX_BLOCKS ? most : DIAG_MAX_BLOCKS);
        k_log_partial<<<grid, DIAG_TB, 0, s>>>(n0, keep, pos, stage, stride, part);
    }
    k_log_final<<<1, DIAG_TB, 0, s>>>(n0, keep, pos, part, step, t,
                                      static_cast<unsigned long long *>(rec));
}

}  // namespace bh
