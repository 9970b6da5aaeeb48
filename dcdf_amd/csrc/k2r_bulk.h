// k2r_bulk.h -- the bulk decoder's work unit and launcher (k2r_bulk.hip), planned by plan_decode (k2r_plan.h).  The structs and
// the split arithmetic compile for the host alone as well (g++).
#pragma once
#if defined(__HIPCC__)
#include "k2r_query_types.h"  // (ChunkRef, for the launcher and for k2r_bulk.hip)
#else
#include "k2r_common.h"
#endif

namespace k2r {

constexpr uint32_t BULK_REGION = 64;  // a unit's region: 64 x 64 cells on the chunk's own 64-grid
// One workgroup's work: the instants [t0, t1) of one chunk over the part [top, bottom) x [left, right) (chunk coordinates,
// half-open, never empty) of the region whose origin is (rr, rc).  The workgroup decodes the Snapshot of every block it meets
// once and each of the block's instants from the Log's own tree.
struct BulkUnit {
    uint32_t chunk;  // index into the ChunkRef table
    uint32_t t0, t1;
    uint16_t rr, rc;
    uint16_t top, bottom, left, right;
    uint32_t out_sr;   // output row stride in elements (column stride 1)
    uint64_t out_st;   // output instant stride in elements
    uint64_t out_off;  // element of cell (t0, top, left) in `out`
};
// instants [t0, t0 + nt) in `parts` pieces: piece j is [bulk_part(j), bulk_part(j + 1))
K2R_HD uint32_t bulk_part(uint32_t t0, uint32_t nt, uint32_t parts, uint32_t j) { return t0 + (uint32_t)((uint64_t)nt * j / parts); }
// Pieces per unit when there are few units: enough workgroups for `wanted` (a few per compute unit), but no piece shorter than
// four instants -- every piece decodes its block's Snapshot again, which costs about as much as one Log instant and a half.
K2R_HD uint32_t bulk_parts(uint64_t n_units, uint32_t nt, uint32_t wanted) {
    if (n_units == 0 || n_units >= wanted) return 1u;
    const uint64_t want = (wanted + n_units - 1) / n_units, cap = nt / 4u;
    const uint64_t p = want < cap ? want : cap;
    return p < 1 ? 1u : (uint32_t)p;
}

#if defined(__HIPCC__)
// k_bulk_decode over n units on the null stream (asynchronous); d_out holds out_dtype elements.  Returns a DCDF code.
int launch_bulk_decode(const ChunkRef* d_refs, const BulkUnit* d_units, uint32_t n, void* d_out, int32_t out_dtype);
// workgroups the device wants in flight before a unit's instants are worth splitting
uint32_t bulk_wanted_units();
#endif

}  // namespace k2r
