// The frame's quadtree overlay on the device (bh_render_quads, include/bh_engine.h): what
// NBodyPanel.paintComponent draws for getTreeForDebug().visitQuads (PNL:326-344), as a plane of
// line-draw counts.  Nothing of the tree goes to the host.
//
// Cells.  QuadWalker (engine.cpp) emits the root, the four children of every cell that holds two
// or more in-root bodies, and under a depth-J jitter cell also the four grandchildren of every
// child in the node record's jmask.  The cell of depth d that holds the sorted bodies lo..hi-1
// (hi - lo >= 2) is found from lo alone: cpl[lo-1] < d <= cpl[lo].  So lane a, one per sorted
// body, owns the cells of depths cpl[a-1]+1 .. min(cpl[a], J) along its own key and emits their
// children; lane 0 also emits the root.  A jitter run's followers have cpl[a-1] == J and own
// nothing.  Cell centres are Quad.child iterated from the root along the key's digits with the
// engine's per-depth h table (h[d+1] = h[d] / 2.0, as BHA:74 computes it): the same operations
// in the same order as the host walk, at most J steps per lane.
//
// Lines.  Cell (cx, cy, h) of depth d draws from x = toInt(((cx - h) - view_x) * zoom),
// y = toInt(((cy - h) - view_y) * zoom) a vertical and a horizontal line of s + 1 pixels,
// s = toInt(h * 2.0 * zoom) from a per-depth table made on the host; x + s and y + s in 64 bits.
// Line lengths run from one pixel to the whole view, so a line is not drawn pixel by pixel: the
// clipped line is +1 at its first pixel and -1 just past its last in a difference plane (rowd for
// horizontal lines, cold for vertical ones; uint32 atomic adds, sums modulo 2^32 of a true count
// below 2^32).  A cell with s == 0 is one pixel drawn twice: +2 in a third plane (dir) instead of
// four difference entries (BH_QUADS_DIRECT=0 sends them through the difference planes too).  A
// lane's cells are nested, and the slots are in Morton order: the +2 of consecutive cells of a
// lane, and then of neighbouring lanes, that fall on one pixel are summed before they go to
// memory (BH_QUADS_COMBINE=0: one atomic per cell).  The switches change no byte of the image.
// k_quad_rows: one workgroup per row, QUADS_ROW_CHUNK columns per iteration with a carry: the
// running sum of rowd plus dir into out.  k_quad_cols: one workgroup per QUADS_COL_TILE columns,
// QUADS_COL_BANDS waves that each take a band of rows -- band totals first, then the running sum
// of cold added into out, QUADS_COL_BATCH rows in flight per lane.  Every read and write of both is a run of consecutive columns of one
// row.  Both write zero back where a working plane was touched.  Integer adds only: the image
// does not depend on arrival order.
#include "render_quads.hpp"

#include <cstdlib>

namespace bh {
namespace {

constexpr int TB = 256;

struct QuadView {
    double view_x, view_y, zoom;
    int32_t width, height;
    int32_t s[MAX_DEPTH_TAB];  // toInt(h[d] * 2.0 * zoom)
};

// Kotlin's Double.toInt()
__host__ __device__ inline int32_t kt_to_int(double d) {
    if (d != d) return 0;
    if (d >= 2147483647.0) return 2147483647;
    if (d <= -2147483648.0) return -2147483647 - 1;
    return (int32_t)d;
}

struct Planes {
    uint32_t *rowd, *cold, *dir;
};

constexpr uint32_t NO_PIXEL = 0xFFFFFFFFu;
// how one-pixel cells (s == 0) are drawn
constexpr int MODE_DIFF = 0;     // as every other cell, through the difference planes
constexpr int MODE_DIRECT = 1;   // one +2 into dir per cell
constexpr int MODE_COMBINE = 2;  // +2 per cell, summed over a lane's and then a wave's runs of
                                 // equal pixels before it goes to dir
struct Pending {  // MODE_COMBINE: the lane's current run
    uint32_t pix = NO_PIXEL, val = 0u;
};

template <int MODE>
__device__ __forceinline__ void draw_cell(double cx, double cy, double h, int32_t s,
                                          const QuadView &q, const Planes &p, Pending &run) {
    const int32_t x = kt_to_int(((cx - h) - q.view_x) * q.zoom);
    const int32_t y = kt_to_int(((cy - h) - q.view_y) * q.zoom);
    const int64_t W = q.width, H = q.height;
    const bool xin = x >= 0 && x < W, yin = y >= 0 && y < H;
    if (MODE != MODE_DIFF && s == 0) {
        if (xin && yin) {
            const uint32_t pix = (uint32_t)y * (uint32_t)q.width + (uint32_t)x;
            if (MODE == MODE_DIRECT) {
                atomicAdd(p.dir + pix, 2u);
            } else if (pix == run.pix) {
                run.val += 2u;
            } else {
                if (run.pix != NO_PIXEL) atomicAdd(p.dir + run.pix, run.val);
                run.pix = pix;
                run.val = 2u;
            }
        }
        return;
    }
    if (xin) {  // drawLine(x, y, x, y + s): rows max(y, 0) .. min(y + s, H - 1)
        const int64_t r0 = y > 0 ? y : 0;
        const int64_t r1 = (int64_t)y + s < H - 1 ? (int64_t)y + s : H - 1;
        if (r0 <= r1) {
            atomicAdd(p.cold + r0 * W + x, 1u);
            if (r1 + 1 < H) atomicAdd(p.cold + (r1 + 1) * W + x, 0xFFFFFFFFu);
        }
    }
    if (yin) {  // drawLine(x, y, x + s, y)
        const int64_t c0 = x > 0 ? x : 0;
        const int64_t c1 = (int64_t)x + s < W - 1 ? (int64_t)x + s : W - 1;
        if (c0 <= c1) {
            atomicAdd(p.rowd + (int64_t)y * W + c0, 1u);
            if (c1 + 1 < W) atomicAdd(p.rowd + (int64_t)y * W + c1 + 1, 0xFFFFFFFFu);
        }
    }
}

// BHA:73-81
__device__ __forceinline__ void child_of(double cx, double cy, double hh, int which, double &ox,
                                         double &oy) {
    ox = (which & 1) ? cx + hh : cx - hh;
    oy = (which & 2) ? cy + hh : cy - hh;
}

template <bool IMAGE, int MODE>
__global__ __launch_bounds__(TB) void k_quad_cells(QuadTree t, Geometry g, QuadView q, Planes p,
                                                   unsigned long long *count) {
    __shared__ double hs[MAX_DEPTH_TAB];
    __shared__ int32_t ss[MAX_DEPTH_TAB];
    __shared__ uint32_t wcells[TB / 64];
    Pending run;
    if (IMAGE) {
        if (threadIdx.x < MAX_DEPTH_TAB) {
            hs[threadIdx.x] = g.h[threadIdx.x];
            ss[threadIdx.x] = q.s[threadIdx.x];
        }
        __syncthreads();
    }
    const int J = g.J;
    const int64_t a = (int64_t)blockIdx.x * TB + threadIdx.x;
    uint32_t cells = 0;
    if (a == 0) {  // the root, whatever it holds
        cells = 1;
        if (IMAGE) draw_cell<MODE>(g.root_cx, g.root_cy, hs[0], ss[0], q, p, run);
    }
    if (a < t.n) {
        const uint64_t key = t.keys[a];
        if (key != sentinel_key(J)) {
            const int cp = a > 0 ? (int)t.cpl[a - 1] : -1;
            const int cc = (int)t.cpl[a];
            const int top = cc < J ? cc : J;
            if (top > cp) {
                uint32_t jmask = 0;
                if (top == J)
                    jmask = (t.nodes[t.base[a] + (uint32_t)(J - cp - 1)].meta >> NODE_JMASK_SHIFT) &
                            0xFu;
                cells += 4u * (uint32_t)(top - cp) + 4u * (uint32_t)__popc(jmask);
                if (IMAGE) {
                    double cx = g.root_cx, cy = g.root_cy;
                    for (int d = 0; d <= top; ++d) {
                        const double hh = hs[d + 1];
                        if (d > cp) {
                            for (int w = 0; w < 4; ++w) {
                                double ox, oy;
                                child_of(cx, cy, hh, w, ox, oy);
                                draw_cell<MODE>(ox, oy, hh, ss[d + 1], q, p, run);
                                if (d == J && ((jmask >> w) & 1u)) {
                                    const double h2 = hs[d + 2];
                                    for (int w2 = 0; w2 < 4; ++w2) {
                                        double gx, gy;
                                        child_of(ox, oy, h2, w2, gx, gy);
                                        draw_cell<MODE>(gx, gy, h2, ss[d + 2], q, p, run);
                                    }
                                }
                            }
                        }
                        if (d < top) {
                            const int digit = (int)((key >> (2 * (J - 1 - d))) & 3u);
                            child_of(cx, cy, hh, digit, cx, cy);
                        }
                    }
                }
            }
        }
    }
    const int lane = (int)(threadIdx.x & 63u);
    if (IMAGE && MODE == MODE_COMBINE) {
        // The lanes' last runs: the slots are in Morton order, so neighbouring lanes end on the
        // same pixel in runs; a segmented scan leaves a run's sum in its last lane, which issues
        // it (k_raster's scheme, render.hip).  Runs the scan does not merge meet in memory.
        const uint32_t prev = __shfl_up(run.pix, 1);
        const uint64_t heads = __ballot(lane == 0 || prev != run.pix);
        bool issue = run.pix != NO_PIXEL;
        if (heads != ~0ull) {  // (wave-uniform) some run is longer than one lane
            const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(run.val, d);
                if (lane - d >= start) run.val += o;
            }
            issue = issue && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
        }
        if (issue) atomicAdd(p.dir + run.pix, run.val);
    }
    // the cell count: one atomic per workgroup, spread over QUADS_COUNT_STRIPES cache lines
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cells += __shfl_xor(cells, o);
    if (lane == 0) wcells[threadIdx.x >> 6] = cells;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int w = 0; w < TB / 64; ++w) tot += wcells[w];
        if (tot)
            atomicAdd(count + (size_t)(blockIdx.x % QUADS_COUNT_STRIPES) * QUADS_COUNT_STRIDE, tot);
    }
}

__global__ __launch_bounds__(QUADS_ROW_CHUNK) void k_quad_rows(int32_t W,
                                                               uint32_t *__restrict__ rowd,
                                                               uint32_t *__restrict__ dir,
                                                               uint32_t *__restrict__ out) {
    constexpr int WAVES = QUADS_ROW_CHUNK / 64;
    __shared__ uint32_t wsum[WAVES];
    const size_t row0 = (size_t)blockIdx.x * (size_t)W;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    uint32_t carry = 0;
    for (int32_t c0 = 0; c0 < W; c0 += QUADS_ROW_CHUNK) {
        const int32_t c = c0 + (int32_t)threadIdx.x;
        uint32_t v = 0;
        if (c < W) {
            v = rowd[row0 + c];
            if (v) rowd[row0 + c] = 0u;
        }
        uint32_t sc = v;  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(sc, d);
            if (lane >= d) sc += o;
        }
        if (lane == 63) wsum[wave] = sc;
        __syncthreads();
        uint32_t pre = carry, tot = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t ws = wsum[w];
            if (w < wave) pre += ws;
            tot += ws;
        }
        if (c < W) {
            uint32_t d2 = 0;
            if (dir) {
                d2 = dir[row0 + c];
                if (d2) dir[row0 + c] = 0u;
            }
            out[row0 + c] = sc + pre + d2;
        }
        carry += tot;
        __syncthreads();
    }
}

__global__ __launch_bounds__(QUADS_COL_TILE *QUADS_COL_BANDS) void k_quad_cols(
    int32_t W, int32_t H, uint32_t *__restrict__ cold, uint32_t *__restrict__ out) {
    static_assert(QUADS_COL_TILE == 64, "one wave per row of a column tile");
    __shared__ uint32_t tot[QUADS_COL_BANDS][QUADS_COL_TILE];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int32_t c = (int32_t)blockIdx.x * QUADS_COL_TILE + lane;
    const int32_t band = (H + QUADS_COL_BANDS - 1) / QUADS_COL_BANDS;
    const int32_t r_lo = wave * band < H ? wave * band : H;
    const int32_t r_hi = r_lo + band < H ? r_lo + band : H;
    uint32_t sum = 0;
    if (c < W)
        for (int32_t r = r_lo; r < r_hi; ++r) sum += cold[(size_t)r * (size_t)W + c];
    tot[wave][lane] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (int w = 0; w < wave; ++w) run += tot[w][lane];
    if (c < W)
        for (int32_t r = r_lo; r < r_hi; r += QUADS_COL_BATCH) {
            // a batch of rows is loaded before any of it is stored: a store between two loads
            // of the same plane would make every row wait for the row before
            uint32_t v[QUADS_COL_BATCH], o[QUADS_COL_BATCH];
#pragma unroll
            for (int k = 0; k < QUADS_COL_BATCH; ++k) {
                const bool in = r + k < r_hi;
                const size_t i = (size_t)(r + k) * (size_t)W + c;
                v[k] = in ? cold[i] : 0u;
                o[k] = in ? out[i] : 0u;
            }
#pragma unroll
            for (int k = 0; k < QUADS_COL_BATCH; ++k) {
                const size_t i = (size_t)(r + k) * (size_t)W + c;
                if (v[k]) cold[i] = 0u;  // (v[k] != 0 only inside the band)
                run += v[k];
                if (run && r + k < r_hi) out[i] = o[k] + run;
            }
        }
}

}  // namespace

void quads_render(const QuadTree &t, const Geometry &g, const bh_view &v, uint32_t *rowd,
                  uint32_t *cold, uint32_t *dir, bool combine, uint32_t *out,
                  unsigned long long *count, hipStream_t s) {
    QuadView q;
    q.view_x = v.view_x;
    q.view_y = v.view_y;
    q.zoom = v.zoom;
    q.width = v.width;
    q.height = v.height;
    for (int d = 0; d < MAX_DEPTH_TAB; ++d) q.s[d] = kt_to_int(g.h[d] * 2.0 * v.zoom);
    const Planes p{rowd, cold, dir};
    const int64_t lanes = t.n > 0 ? t.n : 1;  // (lane 0 emits the root of an empty list)
    const unsigned grid = (unsigned)((lanes + TB - 1) / TB);
    if (!out) {
        k_quad_cells<false, MODE_DIFF><<<grid, TB, 0, s>>>(t, g, q, p, count);
        return;
    }
    if (dir && combine)
        k_quad_cells<true, MODE_COMBINE><<<grid, TB, 0, s>>>(t, g, q, p, count);
    else if (dir)
        k_quad_cells<true, MODE_DIRECT><<<grid, TB, 0, s>>>(t, g, q, p, count);
    else
        k_quad_cells<true, MODE_DIFF><<<grid, TB, 0, s>>>(t, g, q, p, count);
    k_quad_rows<<<(unsigned)v.height, QUADS_ROW_CHUNK, 0, s>>>(v.width, rowd, dir, out);
    k_quad_cols<<<(unsigned)((v.width + QUADS_COL_TILE - 1) / QUADS_COL_TILE),
                  QUADS_COL_TILE * QUADS_COL_BANDS, 0, s>>>(v.width, v.height, cold, out);
}

}  // namespace bh
