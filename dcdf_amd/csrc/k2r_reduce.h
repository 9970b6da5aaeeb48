// k2r_reduce.h -- reduction over time (dcdf_raster_reduce_time_batch): what the planner (k2r_plan.h), the bulk kernel
// (k2r_bulk.hip) and the fold kernels share.  Compiles for the host alone as well (g++).
//
// The contract (include/dcdf_k2r.h): per cell, x[t] = the value the typed fill_window returns with the
// leaf's own encoding, widened to double; MIN / MAX = fmin / fmax over the non-NaN x[t]; SUM = the sequential chain
// s = 0.0, s = s + x[t] in instant order; COUNT = the non-NaN x[t]; MEAN = SUM / COUNT.  The chain's order is what every piece
// of the plan keeps: a cell's instants are only ever added one after the other to the one running sum of its state plane.
#pragma once
#include "k2r_cell_fold.h"

namespace k2r {

// accumulators (the first four bits of the DCDF_REDUCE_* mask; MEAN is made of SUM and COUNT by the finishing kernel)
constexpr uint32_t RA_MIN = 1u, RA_MAX = 2u, RA_SUM = 4u, RA_COUNT = 8u, RA_ALL = 15u, ROP_MEAN = 16u;
K2R_HD uint32_t reduce_live(uint32_t ops) { return (ops & RA_ALL) | ((ops & ROP_MEAN) ? (RA_SUM | RA_COUNT) : 0u); }

// Where accumulator A of a cube lives (state_plane, k2r_cell_fold.h): SUM or COUNT kept for MEAN alone are the scratch planes.
K2R_HD double* reduce_plane(uint32_t A, double* dst, double* scr, uint32_t ops, uint64_t o_off, uint64_t s_off, uint64_t psz) {
    return state_plane(A, reduce_live(ops), dst, scr, ops, o_off, s_off, psz);
}

// x[t]: store_typed (k2r_decode.h) of the stored integer n with the leaf's encoding, widened to double
K2R_HD double reduce_widen(int32_t enc, uint32_t fbits, int64_t n) {
    switch (enc) {
        case ENC_I32: return (double)(int32_t)n;
        case ENC_I64: return (double)n;
        case ENC_F32: return n == 0 ? __builtin_nan("") : (double)from_fixed_f32(n, fbits);
        default: return n == 0 ? __builtin_nan("") : from_fixed_f64(n, fbits);
    }
}

// One workgroup's work in k_bulk_reduce: CellUnit (k2r_cell_fold.h), then the place of its cells in the state planes.
struct ReduceUnit : CellUnit {
    uint64_t o_off, s_off, psz;  // of cell (top, left): reduce_plane
};
// A fallback or elided piece: the shared head is all reduce_time needs.
using FoldPiece = CellFold;
K2R_PIN_BEGIN
static_assert(sizeof(ReduceUnit) == 56, "ReduceUnit");
K2R_PIN(ReduceUnit, init, 28) K2R_PIN(ReduceUnit, o_off, 32) K2R_PIN(ReduceUnit, s_off, 40) K2R_PIN(ReduceUnit, psz, 48)
K2R_PIN_END
// MEAN of one cube
struct MeanPiece {
    uint64_t o_off, s_off, psz;
};

#if defined(__HIPCC__)
struct ChunkRef;
// k_bulk_reduce over n units on the null stream (asynchronous).  d_enc: the chunks' encodings.  Returns a DCDF code.
int launch_bulk_reduce(const ChunkRef* d_refs, const uint8_t* d_enc, const ReduceUnit* d_units, uint32_t n, double* d_dst, double* d_scr,
                       uint32_t ops);
#endif

}  // namespace k2r
