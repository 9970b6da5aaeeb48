// k2r_items.h -- the wave walks' work item and the host arithmetic that makes items of a cube.  No device code: the query units
// get it through k2r_query_types.h, the planner (k2r_plan.h) and its CPU check include it with plain g++.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/dcdf_k2r.h"
#include "k2r_common.h"

namespace k2r {

// one (chunk, instant, sub-window) of a wave walk: at most 32 x 32 cells (k_window_wave, k_search_wave) or 64 x 64 (k_window_wave2)
struct WinItem {
    uint32_t chunk, inst;
    uint16_t top, bottom, left, right;  // sub-window, chunk coordinates, half-open
    uint32_t out_sr;                     // output row stride in elements (column stride 1)
    uint64_t out_off;                    // element offset of cell (top, left) of this instant in `out`
};

// geom::Cube::new reorders reversed bounds (geom.rs:83-103)
inline dcdf_cube norm_cube(const dcdf_cube& c) {
    dcdf_cube o = c;
    if (o.start > o.end) std::swap(o.start, o.end);
    if (o.top > o.bottom) std::swap(o.top, o.bottom);
    if (o.left > o.right) std::swap(o.left, o.right);
    return o;
}
inline uint64_t cube_cells(const dcdf_cube& c) { return (uint64_t)(c.end - c.start) * (c.bottom - c.top) * (c.right - c.left); }  // (normalised)
// wave items along one axis of a piece [a, b) in chunk coordinates: from the piece's start (node-wise walk, step 64) or from the
// chunk's 32-grid (step 32) -- the loops of window_items / k_raster_expand / k_raster_tiled_expand
K2R_HD uint32_t axis_items(uint32_t a, uint32_t b, uint32_t step) { return (b - (step == 64 ? a : (a & ~31u)) + step - 1) / step; }
// (chunk, instant, sub-window) items of one chunk-level cube `c`: pieces of at most 64 x 64 cells from the window's origin
// (node_wise: k_window_wave2), else the squares of the chunk's 32-grid the window meets (k_window_wave, k_search_wave), so that a
// frontier level never exceeds what a wave's LDS queue holds.  out_base = element offset of cell (c.start, c.top, c.left);
// sr / st = row and instant strides of the array the window is written into (0 = the window's own dense layout; a piece of a
// larger window passes the parent's)
inline void window_items(uint32_t chunk, const dcdf_cube& c, uint64_t out_base, std::vector<WinItem>& items, bool node_wise, uint64_t sr = 0,
                         uint64_t st = 0) {
    const uint64_t wc = sr ? sr : (uint64_t)(c.right - c.left), wr_wc = st ? st : (uint64_t)(c.bottom - c.top) * wc;
    const uint32_t step = node_wise ? 64u : 32u;
    for (uint32_t t = c.start; t < c.end; t++)
        for (uint32_t r = node_wise ? c.top : (c.top & ~31u); r < c.bottom; r += step)
            for (uint32_t cc = node_wise ? c.left : (c.left & ~31u); cc < c.right; cc += step) {
                WinItem it{};
                it.chunk = chunk;
                it.inst = t;
                it.top = (uint16_t)std::max(r, c.top);
                it.bottom = (uint16_t)std::min(r + step, c.bottom);
                it.left = (uint16_t)std::max(cc, c.left);
                it.right = (uint16_t)std::min(cc + step, c.right);
                it.out_sr = (uint32_t)wc;
                it.out_off = out_base + (uint64_t)(t - c.start) * wr_wc + (uint64_t)(it.top - c.top) * wc + (it.left - c.left);
                items.push_back(it);
            }
}

}  // namespace k2r
