// k2r_session.h -- the encode session as the units of the encode side see it (k2r_capi_encode.hip owns it; k2r_host_batch.hip
// and k2r_superchunk.hip read a finished one).
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "k2r_runtime.h"
#include "k2r_session_plan.h"

// dcdf_encoder = a device-resident encode session: tile descriptors, per-tile output slots, per-class work queues.
struct dcdf_encoder {
    std::vector<dcdf_tile_desc> desc;
    k2r::SessionPlan plan;                  // what runs where (k2r_session_plan.h); its offsets are pointers in `args`
    std::vector<k2r::TileArgs> args;        // host mirror of the device array: plan.items as the kernels read them
    std::vector<k2r::TileResult> results;   // host copy after run
    k2r::DevBuf d_args, d_results, d_out, d_minmax, d_order, d_queue, d_lists;
    std::vector<std::unique_ptr<k2r::DevBuf>> retry_slots;  // bigger slots for tiles that overflowed
    // Speculative parts (k2r_encode.h): tiles encoded as several work items, the tile's own TileArgs restricted to the first
    // instants and extra TileArgs at indices >= n for the rest, spliced by k_stitch inside the timed region.
    bool spliced = true;     // false between a run and the first request for a split tile's bytes
    k2r::PartTables splice;  // the split tiles whose parts checked out in the last run (splice_tables)
    k2r::DevBuf d_part_first, d_part_items, d_out_b, d_flags, d_shared;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~dcdf_encoder() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) k2r::StreamPool::get().give(false, stream);
    }
};

#define K2R_TRY(call)                    \
    do {                                 \
        const int _rc = (call);          \
        if (_rc != DCDF_OK) return _rc;  \
    } while (0)

namespace k2r {

// tile i was accepted on the host and encoded by the last run
inline bool tile_ok(const dcdf_encoder* e, size_t i) { return e->plan.pre_status[i] == DCDF_OK && e->results[i].status == ST_OK; }

// The bytes of the tiles that were encoded in parts, made contiguous in the first part's slot (k_stitch<true>): once per run,
// the first time they are asked for.
int materialize(dcdf_encoder* e);

// The encoded bytes of a finished session, device slots -> pinned double buffer -> wherever `dst(tile, len)` says (called once
// per tile with bytes, from worker threads; it may allocate the destination there).  k2r_host_batch.hip.
// `landed(tile)`, if given, runs on the worker thread right after a tile's bytes have been copied to their destination.
int encoder_download(dcdf_encoder* e, const std::function<uint8_t*(size_t, uint64_t)>& dst,
                     const std::function<void(size_t)>& landed = nullptr);

}  // namespace k2r
