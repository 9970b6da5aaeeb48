// k2r_raster_host.h -- the raster handle and what its two translation units share: k2r_raster.hip (constructors, fill_window,
// search, get / fill_cell) and k2r_raster_region.hip (the region calls: decode, reduce_time, reduce_time_groups, moments_time, moments_time_groups, spells, quantile_time,
// regress_time, regress_time_groups, rolling_time, rolling_time_groups, reduce_space, histogram, zonal).  Host code only.
#pragma once
#include "k2r_plan.h"
#include "k2r_query_host.h"

// one leaf of a tiled raster (dcdf_raster_tile without its pointers): where the leaf starts inside its chunk, or the elided
// leaf's encoding / bits (its values live in dcdf_raster::d_vals), and what its holding node's (min, max) allow
struct RasterLeaf {
    uint32_t row0, col0;
    int32_t enc;          // of the values / minmax
    uint8_t elided, fbits, has_mm, exact;
};
struct dcdf_raster {
    std::vector<dcdf_chunk*> chunks;  // [(segment * nti + ti) * ntj + tj]
    // d_refs holds device pointers into the chunks' streams and tables: the raster shares the ownership of every slab a batch-opened
    // chunk lives in (dcdf_chunk::store), so closing such a chunk first leaves the raster usable; chunks opened one by one own their
    // buffers themselves and must outlive the raster (dcdf_k2r.h)
    std::vector<std::shared_ptr<void>> keep;
    uint32_t T = 0, R = 0, C = 0, tile = 0, cs = 0, nseg = 0, nti = 0, ntj = 0;
    k2r::DevBuf d_refs;
    k2r::DevBuf d_quirk;  // [chunk][chunk_size]: dcdf_chunk::search_quirk of every instant (k_raster_search_expand)
    k2r::DevBuf d_enc;    // [chunk]: the chunk's encoding (value search translates its bounds per piece on the device)
    bool all_wave = true, all_node = true, all_narrow = true;
    bool bad_fbits = false;  // a float chunk with fractional bits value_bounds does not take (> 62)
    // tiled rasters (dcdf_raster_create_tiles): the grid is one of leaves; chunks[] / d_refs hold NULL / zeros for elided leaves
    // and the all_* flags are over chunk leaves only
    bool tiled = false;
    std::vector<RasterLeaf> leaves;  // [leaf]
    k2r::DevBuf d_leaf;              // the same on the device
    k2r::DevBuf d_vals;              // [leaf][chunk_size] int64: an elided leaf's value per instant (0 elsewhere)
    k2r::DevBuf d_mm;                // [leaf][chunk_size][2] int64: the holding node's (min, max) per instant (RasterLeaf::has_mm)
    std::vector<k2r::PlanLeaf> plan_leaves;  // [leaf], plain and tiled rasters alike: all the planner (k2r_plan.h) knows of a leaf
    k2r::PlanRaster plan() const { return k2r::PlanRaster{T, R, C, tile, cs, nti, ntj, plan_leaves.data()}; }
};

namespace k2r {

// k_raster_fill_const (k2r_raster.hip) over n elided pieces on the null stream (asynchronous).  Returns a DCDF code.
int launch_raster_fill_const(const dcdf_raster* r, const ConstPiece* d_consts, uint32_t n, void* d_out, int32_t out_dtype);

// The end of every batch call: e1 recorded and the device idle (record = false: a walk launch has done both), the host form's
// windows moved to the caller's array, the time between the events reported.
inline int batch_epilogue(const WindowOut& W, const EventPair& ev, bool record, float* kernel_ms) {
    if (record) {
        K2R_HIP(hipEventRecord(ev.e1, 0));
        K2R_HIP(hipDeviceSynchronize());
    }
    const int rc = W.finish();
    if (rc != DCDF_OK) return rc;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}

}  // namespace k2r
