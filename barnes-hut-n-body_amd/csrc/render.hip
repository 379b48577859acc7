// The frame's body pass on the device (bh_render_bodies, include/bh_engine.h): what
// NBodyPanel.paintComponent's loop over engine.getBodies() paints (PNL:302-307), as an image.
//
// Body i of the caller's list is drawn at
//     sx = toInt((x_i - view_x) * zoom),  sy = toInt((y_i - view_y) * zoom)      (binary64)
// iff 0 <= sx < width && 0 <= sy < height, Kotlin's Double.toInt(): NaN -> 0, else truncation
// toward zero (saturating).  The test is made in double -- drawn iff t is NaN or -1 < t < size --
// so the conversion is only ever applied to a value in (-1, size).  A later body of the list
// overwrites an earlier one: the pixel belongs to the largest caller index drawn on it.
//
// k_raster: one lane per slot; one uint32 atomic max of ((cidx + 1) << 1) | (m >= heavy_mass) into
// the packed plane (the maximum is the maximum over cidx, the low bit is the winner's colour) and,
// when the density is asked for, one uint32 atomic add into the count plane.  Integer max and add
// only: the planes do not depend on arrival order.  The slots are in Morton order, so the lanes
// of a wave fall on few pixels in runs; a segmented scan over each run of equal pixels leaves the
// run's max in its last lane, which issues the run's two atomics.  Runs that the scan does not
// merge (equal pixels that are not neighbours) meet in memory: the result is the same.
// k_resolve: one lane per 4 pixels; unpacks into the staged planes asked for with 16-byte (4-byte
// for the uint8 plane) stores and writes 0 back where the working planes were touched, so they
// are zero again when the call ends and no fill runs between calls.
#include "bh_device.hpp"

#include <cstdlib>

namespace bh {
namespace {

constexpr int TB = 256;
constexpr uint32_t NO_PIXEL = 0xFFFFFFFFu;

template <bool COMBINE, bool COUNTS>
__global__ __launch_bounds__(TB) void k_raster(int64_t n, const double *__restrict__ x,
                                               const double *__restrict__ y,
                                               const double *__restrict__ m,
                                               const uint32_t *__restrict__ cidx, bh_view v,
                                               uint32_t *__restrict__ packed,
                                               uint32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    uint32_t pix = NO_PIXEL, val = 0u;
    if (i < n) {
        const uint32_t c = cidx ? cidx[i] : (uint32_t)i;  // (no cidx: the list's own order)
        if (!(c & CIDX_DEAD)) {
            const double tx = (x[i] - v.view_x) * v.zoom;
            const double ty = (y[i] - v.view_y) * v.zoom;
            const bool nx = tx != tx, ny = ty != ty;
            if ((nx || (tx > -1.0 && tx < (double)v.width)) &&
                (ny || (ty > -1.0 && ty < (double)v.height))) {
                const int32_t sx = nx ? 0 : (int32_t)tx;  // in (-1, width): the cast is defined
                const int32_t sy = ny ? 0 : (int32_t)ty;
                pix = (uint32_t)sy * (uint32_t)v.width + (uint32_t)sx;
                val = ((c + 1u) << 1) | (m && m[i] >= v.heavy_mass ? 1u : 0u);
            }
        }
    }
    uint32_t count = 1u;
    bool issue = pix != NO_PIXEL;
    if (COMBINE) {
        // runs of equal pixels (undrawn lanes form runs of their own that issue nothing)
        const int lane = (int)(threadIdx.x & 63u);
        const uint32_t prev = __shfl_up(pix, 1);
        const uint64_t heads = __ballot(lane == 0 || prev != pix);
        if (heads != ~0ull) {  // (wave-uniform) some run is longer than one lane
            const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(val, d);
                if (lane - d >= start) val = o > val ? o : val;
            }
            count = (uint32_t)(lane - start + 1);
            issue = issue && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
        }
    }
    if (issue) {
        atomicMax(packed + pix, val);
        if (COUNTS) atomicAdd(cnt + pix, count);
    }
}

__global__ __launch_bounds__(TB) void k_resolve(uint32_t quads, uint4 *__restrict__ packed,
                                                uint4 *__restrict__ cnt,
                                                uint32_t *__restrict__ pixels,
                                                uint4 *__restrict__ owner,
                                                uint4 *__restrict__ counts) {
    const uint32_t q = blockIdx.x * TB + threadIdx.x;
    if (q >= quads) return;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const uint4 p = packed[q];
    if (p.x | p.y | p.z | p.w) packed[q] = zero;
    if (pixels) {
        // 0 nothing, 1 white, 2 black: byte k is pixel 4 q + k
        const uint32_t b0 = p.x ? 1u + (p.x & 1u) : 0u, b1 = p.y ? 1u + (p.y & 1u) : 0u;
        const uint32_t b2 = p.z ? 1u + (p.z & 1u) : 0u, b3 = p.w ? 1u + (p.w & 1u) : 0u;
        pixels[q] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
    // (0 >> 1) - 1 = 0xFFFFFFFF: nothing drawn
    if (owner) owner[q] = make_uint4((p.x >> 1) - 1u, (p.y >> 1) - 1u, (p.z >> 1) - 1u,
                                     (p.w >> 1) - 1u);
    if (cnt) {
        const uint4 c = cnt[q];
        if (c.x | c.y | c.z | c.w) cnt[q] = zero;
        counts[q] = c;
    }
}

}  // namespace

size_t render_padded_pixels(int32_t width, int32_t height) {
    return ((size_t)width * (size_t)height + 3) / 4 * 4;
}

void render_raster(int64_t n, const double *x, const double *y, const double *m,
                   const uint32_t *cidx, const bh_view &v, uint32_t *packed, uint32_t *cnt,
                   hipStream_t s) {
    if (n <= 0) return;
    // BH_RENDER_COMBINE=0: every drawn lane issues its own atomics (A/B; the same bytes).  Read
    // per call, so that one process can interleave the two (tools/render_bench.py).
    const char *env = std::getenv("BH_RENDER_COMBINE");
    const bool combine = env ? std::atoi(env) != 0 : true;
    const unsigned grid = (unsigned)((n + TB - 1) / TB);
    if (combine) {
        if (cnt)
            k_raster<true, true><<<grid, TB, 0, s>>>(n, x, y, m, cidx, v, packed, cnt);
        else
            k_raster<true, false><<<grid, TB, 0, s>>>(n, x, y, m, cidx, v, packed, cnt);
    } else {
        if (cnt)
            k_raster<false, true><<<grid, TB, 0, s>>>(n, x, y, m, cidx, v, packed, cnt);
        else
            k_raster<false, false><<<grid, TB, 0, s>>>(n, x, y, m, cidx, v, packed, cnt);
    }
}

void render_resolve(size_t padded_pixels, uint32_t *packed, uint32_t *cnt, uint8_t *pixels,
                    uint32_t *owner, uint32_t *counts, hipStream_t s) {
    const uint32_t quads = (uint32_t)(padded_pixels / 4);
    if (quads == 0) return;
    k_resolve<<<(quads + TB - 1) / TB, TB, 0, s>>>(
        quads, reinterpret_cast<uint4 *>(packed), reinterpret_cast<uint4 *>(cnt),
        reinterpret_cast<uint32_t *>(pixels), reinterpret_cast<uint4 *>(owner),
        reinterpret_cast<uint4 *>(counts));
}

}  // namespace bh
