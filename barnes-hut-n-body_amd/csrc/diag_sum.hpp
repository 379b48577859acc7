// The fixed-order sums of the global diagnostics, shared by the kernels that make them
// (potential.hip diag_reduce for bh_compute_diagnostics, step_log.hip for the step log's records):
// one partition, one per-thread order and one LDS tree, so that both return identical bits for
// the same list.
//
// Sums over the bodies in the caller's list order (the engine stages the state there first), so
// the result depends on the list alone, not on the slot order of the last build: thread t of
// workgroup g adds the bodies g * CHUNK + t, + DIAG_TB, ... in ascending order, the workgroup's
// threads are combined by a fixed tree in LDS, and one final workgroup adds the partials the
// same way.  Two calls on the same state therefore return identical bits.
#pragma once
#include "bh_device.hpp"

namespace bh {

constexpr int DIAG_TB = 256;
constexpr int DIAG_K = 8;           // mass, mx, my, px, py, lz, kinetic, sum m * phi
constexpr int DIAG_MAX_BLOCKS = 1024;

// The partition of n bodies: whole workgroup strides per chunk, at most DIAG_MAX_BLOCKS chunks
// (n = 0: one, all zeros).
struct DiagPartition {
    int64_t chunk;
    int blocks;
};
__host__ __device__ inline DiagPartition diag_partition(int64_t n) {
    int64_t chunk = (n + DIAG_MAX_BLOCKS - 1) / DIAG_MAX_BLOCKS;
    chunk = (chunk + DIAG_TB - 1) / DIAG_TB * DIAG_TB;
    if (chunk < DIAG_TB) chunk = DIAG_TB;
    const int blocks = (int)((n + chunk - 1) / chunk) > 0 ? (int)((n + chunk - 1) / chunk) : 1;
    return DiagPartition{chunk, blocks};
}

#ifdef __HIPCC__
__device__ __forceinline__ void block_tree_sum(double (&v)[DIAG_K], double (*lds)[DIAG_TB]) {
    for (int k = 0; k < DIAG_K; ++k) lds[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = DIAG_TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < DIAG_K; ++k) lds[k][threadIdx.x] += lds[k][threadIdx.x + w];
        __syncthreads();
    }
}

// Workgroup `block` of the partition: its chunk's partial sums into part[block * DIAG_K ..].
__device__ __forceinline__ void diag_partial_block(int block, int64_t n, int64_t chunk,
                                                   const double *__restrict__ x,
                                                   const double *__restrict__ y,
                                                   const double *__restrict__ vx,
                                                   const double *__restrict__ vy,
                                                   const double *__restrict__ m,
                                                   const double *__restrict__ phi,
                                                   double *__restrict__ part,
                                                   double (*lds)[DIAG_TB]) {
    double v[DIAG_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t lo = (int64_t)block * chunk;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += DIAG_TB) {
        const double xi = x[i], yi = y[i], vxi = vx[i], vyi = vy[i], mi = m[i];
        v[0] += mi;
        v[1] += mi * xi;
        v[2] += mi * yi;
        v[3] += mi * vxi;
        v[4] += mi * vyi;
        v[5] += mi * (xi * vyi - yi * vxi);
        v[6] += 0.5 * mi * (vxi * vxi + vyi * vyi);
        if (phi) v[7] += mi * phi[i];
    }
    block_tree_sum(v, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < DIAG_K; ++k) part[(size_t)block * DIAG_K + k] = lds[k][0];
}

// The final workgroup: the sums of `blocks` partials, left in lds[k][0] for every thread to read.
__device__ __forceinline__ void diag_final_block(int blocks, const double *__restrict__ part,
                                                 double (*lds)[DIAG_TB]) {
    double v[DIAG_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = threadIdx.x; g < blocks; g += DIAG_TB)
        for (int k = 0; k < DIAG_K; ++k) v[k] += part[(size_t)g * DIAG_K + k];
    block_tree_sum(v, lds);
}
#endif

}  // namespace bh
