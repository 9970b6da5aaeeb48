// k2r_cell_fold.h -- per-cell folds over time (reduce_time: k2r_reduce.h, reduce_time_groups: k2r_group.h, moments_time: k2r_moment.h, spells: k2r_spell.h): what every such statistic shares
// in the planner (k2r_plan.h), the bulk kernels (k2r_bulk.hip) and the fold kernel (k2r_raster_region.hip).  Compiles for the host
// alone as well (g++).
//
// A cell keeps a small state in output or scratch planes.  Every piece of the plan loads that state (or initialises it when the
// piece holds its cube's first instant), steps through its instants in order and stores the state back; the pieces of a cell
// run one after the other (SegmentPlan), so the result depends on no cut of the cell's instants.  A statistic is a state with
// init, load, step and store (k_cell_fold's Op, k2r_raster_region.hip), two records that begin with the heads below, and a bulk
// kernel of its own on the shared walk (k_bulk_reduce, k_bulk_group, k_bulk_moment, k_bulk_spell: k2r_bulk.hip).
#pragma once
#include <cstddef>

#include "k2r_decode.h"

namespace k2r {

// Where state A of a cube lives: in its own output plane when the caller asked for it (ops; planes in ascending bit order), else
// -- a state kept for another's sake, `live` less `ops` -- in a scratch plane.  o_off / s_off: element of a cell in the cube's
// first output / scratch plane; psz: cells of a plane.
template <class T>
K2R_HD T* state_plane(uint32_t A, uint32_t live, T* dst, T* scr, uint32_t ops, uint64_t o_off, uint64_t s_off, uint64_t psz) {
    if (ops & A) return dst + o_off + (uint64_t)popc32(ops & (A - 1u)) * psz;
    return scr + s_off + (uint64_t)popc32(live & ~ops & (A - 1u)) * psz;
}

// The head of one workgroup's work in a bulk kernel: BulkUnit's first 24 bytes (k2r_bulk.h), then the row stride of the state
// planes.  init: the piece starts at its cube's first instant -- the state is initialised, not loaded.  A unit record ends with
// o_off, s_off, psz of its cell (top, left): state_plane.
struct CellUnit {
    uint32_t chunk;  // index into the ChunkRef table
    uint32_t t0, t1;
    uint16_t rr, rc;
    uint16_t top, bottom, left, right;
    uint32_t sr;  // row stride of the planes in elements (the cube's columns)
    uint32_t init;
};
// The head of a fallback or elided piece folded by k_cell_fold, a thread per cell looping over the instants in order.  src:
// element of (first instant, first row, first column) in the slab of stored integers, dense [nt][rows][cols]; for an elided piece
// the index of its first instant in dcdf_raster::d_vals (one value per instant).
struct CellFold {
    uint32_t nt, rows, cols, sr, init;
    int32_t enc;
    uint32_t fbits, elided;
    uint64_t src, o_off, s_off, psz;
};

// The device reads the records as the planner wrote them: every record pins its size and K2R_PIN(record, field, offset) each of
// its fields.  (offsetof into a struct with a base is conditionally supported; both compilers of this project support it and
// warn, hence K2R_PIN_BEGIN / K2R_PIN_END around the pins.)
#define K2R_PIN(S, f, at) static_assert(offsetof(S, f) == at, #S "::" #f " moved");
#define K2R_PIN_BEGIN _Pragma("GCC diagnostic push") _Pragma("GCC diagnostic ignored \"-Winvalid-offsetof\"")
#define K2R_PIN_END _Pragma("GCC diagnostic pop")

K2R_PIN_BEGIN
static_assert(sizeof(CellUnit) == 32 && sizeof(CellFold) == 64, "the record heads");
K2R_PIN(CellUnit, chunk, 0) K2R_PIN(CellUnit, t0, 4) K2R_PIN(CellUnit, t1, 8) K2R_PIN(CellUnit, rr, 12) K2R_PIN(CellUnit, rc, 14)
K2R_PIN(CellUnit, top, 16) K2R_PIN(CellUnit, bottom, 18) K2R_PIN(CellUnit, left, 20) K2R_PIN(CellUnit, right, 22)
K2R_PIN(CellUnit, sr, 24) K2R_PIN(CellUnit, init, 28)
K2R_PIN(CellFold, nt, 0) K2R_PIN(CellFold, rows, 4) K2R_PIN(CellFold, cols, 8) K2R_PIN(CellFold, sr, 12) K2R_PIN(CellFold, init, 16)
K2R_PIN(CellFold, enc, 20) K2R_PIN(CellFold, fbits, 24) K2R_PIN(CellFold, elided, 28) K2R_PIN(CellFold, src, 32)
K2R_PIN(CellFold, o_off, 40) K2R_PIN(CellFold, s_off, 48) K2R_PIN(CellFold, psz, 56)
K2R_PIN_END

}  // namespace k2r
