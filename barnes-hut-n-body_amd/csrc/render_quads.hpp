// Launchers and tile constants of the quadtree overlay (render_quads.hip, bh_render_quads).
// tests/test_gpu_render_quads.py reads the four QUADS_ROW_* / QUADS_COL_* constants from this
// file to place view sizes on the edges of the scans' tiles: keep them plain `constexpr int NAME = value;` lines.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "bh_device.hpp"

namespace bh {

constexpr int QUADS_ROW_CHUNK = 256;  // columns one workgroup scans per iteration of a row
constexpr int QUADS_COL_TILE = 64;    // columns per workgroup of the column scan (one wave wide)
constexpr int QUADS_COL_BANDS = 16;   // row bands (waves) per workgroup of the column scan
constexpr int QUADS_COL_BATCH = 8;    // rows of its band a lane of the column scan has in flight
// the cell count is accumulated in QUADS_COUNT_STRIPES partial sums, one cache line apart
constexpr int QUADS_COUNT_STRIPES = 32;
constexpr int QUADS_COUNT_STRIDE = 16;  // in 8-byte words
constexpr int QUADS_COUNT_WORDS = QUADS_COUNT_STRIPES * QUADS_COUNT_STRIDE;

// The tree of the last build as QuadWalker (engine.cpp) reads it, all on the device.
struct QuadTree {
    const uint64_t *keys;  // sorted keys, n entries (sentinels last)
    const int8_t *cpl;     // common digits of sorted keys a, a + 1
    const uint32_t *base;  // node slot scan
    const Node *nodes;
    int64_t n;
};

// Working planes of width * height uint32 each, zero on entry and zero again on return: rowd (+1
// at a horizontal line's first pixel, -1 past its last), cold (the same down the columns), dir
// (+2 per cell whose lines are one pixel; null: those go through rowd / cold too; combine: runs
// of equal pixels are summed in the lane and the wave first).  out: the count plane, width *
// height.  count (device, QUADS_COUNT_WORDS 8-byte words, zero on entry): the number of cells is
// the sum of its words.  out == null: the count only -- no plane is read or written.
void quads_render(const QuadTree &t, const Geometry &g, const bh_view &v, uint32_t *rowd,
                  uint32_t *cold, uint32_t *dir, bool combine, uint32_t *out,
                  unsigned long long *count, hipStream_t s);

}  // namespace bh
