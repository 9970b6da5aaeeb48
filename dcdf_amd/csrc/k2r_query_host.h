// k2r_query_host.h -- host side of the query translation units: the chunk handle (k2r_open.hip makes it), the small helpers every
// entry point uses, and what the raster layer (k2r_raster.hip) calls in the walk unit (k2r_query.hip).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "k2r_query_types.h"
#include "k2r_runtime.h"

struct dcdf_chunk {
    // one per instant, stream order == instant order.  A chunk opened from device memory (dcdf_chunk_open_batch) has them on
    // the device only; the few host-side readers fetch them on first use (host_descs)
    mutable std::vector<k2r::InstDesc> descs;
    mutable std::once_flag descs_once;
    uint32_t k0 = 0, sidelen0 = 0;  // of instant 0 (== every instant's)
    uint32_t instants = 0, rows = 0, cols = 0, n_blocks = 0;
    int32_t encoding = 0;
    uint32_t fbits = 0;
    size_t len = 0;
    k2r::DevBuf d_bytes, d_descs;
    // where the device-side views live: the chunk's own buffers (dcdf_chunk_open) or a slab shared by a batch
    // (dcdf_chunk_open_batch); make_ref() reads only these
    const uint8_t* p_bytes = nullptr;
    const k2r::InstDesc* p_descs = nullptr;
    const void* p_top = nullptr;
    const void* p_top_mm = nullptr;
    std::shared_ptr<void> store;  // keeps a batch's slab alive until its last chunk is closed
    // k = 2, sidelen 32..256: for every instant the walk's state at each node of side 16 (k_top_table, built at open): the wave
    // walks of fill_window / search start there instead of at the root (an item begins with
    // the entries of the squares it meets)
    k2r::DevBuf d_top, d_top_mm;
    uint32_t top_g = 0;  // squares per side (sidelen / 16), 0 = no table
    // every stored value of every instant lies in [-2^30, 2^30) (from the root extremes): the query walks then run on 32-bit
    // values (NodeStT<int32_t>).  (A crafted chunk whose inner Dac values contradict its roots decodes to different garbage than
    // with 64-bit arithmetic; no address depends on a value.)
    bool narrow32 = false;
    // per instant: a single-node UNIFORM log over a multi-node snapshot.  The reference's search (log.rs:519-702) never reads
    // eqB[0] and descends the snapshot with the log's (min, max) pair as if it were "equal": its result there is not the set of
    // cells in range, so such instants are searched by the per-thread replica of that descent, not by the decoding wave walk.
    std::vector<uint8_t> search_quirk;
};

namespace k2r {

// the host copy of a chunk's instant descriptors
inline const std::vector<InstDesc>& host_descs(const dcdf_chunk* h) {
    std::call_once(h->descs_once, [h] {
        if (h->descs.empty() && h->p_descs && h->instants) {
            h->descs.resize(h->instants);
            if (hipMemcpy(h->descs.data(), h->p_descs, (size_t)h->instants * sizeof(InstDesc), hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                h->descs.clear();
            }
        }
    });
    return h->descs;
}
inline ChunkRef make_ref(const dcdf_chunk* h) {
    return ChunkRef{h->p_bytes, h->p_descs, h->instants, h->rows, h->cols, h->fbits,
                    h->top_g ? (const TopEnt*)h->p_top : nullptr, h->top_g ? (const TopMM*)h->p_top_mm : nullptr, h->top_g, 0};
}
inline bool cube_in(const dcdf_chunk* h, const dcdf_cube& c) {  // mmarray.rs:218-229
    return c.end <= h->instants && c.bottom <= h->rows && c.right <= h->cols;
}
// the wave kernel handles k * k <= 64 children per node and 16-bit coordinates
inline bool wave_kernel_ok(const dcdf_chunk* h) { return h->k0 * h->k0 <= 64 && h->sidelen0 <= 65535; }
inline bool node_kernel_ok(const dcdf_chunk* h) { return h->k0 == 2 && h->sidelen0 >= 4; }
inline bool out_args_ok(int32_t out_dtype, int out_mem) {
    return (out_dtype == DCDF_I32 || out_dtype == DCDF_I64 || out_dtype == DCDF_F32 || out_dtype == DCDF_F64) &&
           (out_mem == DCDF_MEM_HOST || out_mem == DCDF_MEM_DEVICE);
}
inline size_t elem_size(int32_t out_dtype) { return (out_dtype == DCDF_I32 || out_dtype == DCDF_F32) ? 4 : 8; }

struct EventPair {  // destroyed on every exit path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() {
        hipError_t r = hipEventCreate(&e0);
        return r != hipSuccess ? r : hipEventCreate(&e1);
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// a fresh device buffer holding a copy of n host bytes
inline hipError_t upload(DevBuf& d, const void* src, size_t n) {
    const hipError_t e = d.alloc(n);
    return e != hipSuccess ? e : hipMemcpy(d.p, src, n, hipMemcpyHostToDevice);
}
template <class T>
inline hipError_t upload(DevBuf& d, const std::vector<T>& v) { return upload(d, v.data(), v.size() * sizeof(T)); }

// Where the windows of a batch of cubes go.  Device output: cube q's window is written by the kernels at out_offset[q] (elements)
// of the caller's array.  Host output: the windows are decoded back to back into `stage` (the caller allocates total * es bytes)
// and finish() moves them -- one copy when the caller's offsets are the same dense layout (the usual case), else window by
// window: cube q touches out[out_offset[q] .. + its cell count) and nothing else.
struct WindowOut {
    const dcdf_cube* cubes;
    size_t nq;
    void* out;
    const uint64_t* out_offset;
    size_t es;
    bool to_dev;
    std::vector<uint64_t> base;  // [q]: element of the window's first cell in dst()
    uint64_t total = 0;          // cells of all the windows
    bool dense = true;
    DevBuf stage;
    WindowOut(const dcdf_cube* cubes_, size_t nq_, void* out_, const uint64_t* out_offset_, size_t es_, bool to_dev_)
        : cubes(cubes_), nq(nq_), out(out_), out_offset(out_offset_), es(es_), to_dev(to_dev_), base(nq_) {
        for (size_t q = 0; q < nq; q++) {
            dense = dense && out_offset[q] == total + out_offset[0];
            base[q] = to_dev ? out_offset[q] : total;
            total += cube_cells(norm_cube(cubes[q]));
        }
    }
    void* dst() const { return to_dev ? out : stage.p; }
    int finish() const {  // after the kernels are done
        if (to_dev) return DCDF_OK;
        if (dense) {
            K2R_HIP(hipMemcpy((uint8_t*)out + out_offset[0] * es, stage.p, total * es, hipMemcpyDeviceToHost));
            return DCDF_OK;
        }
        std::vector<uint8_t> tmp(total * es);
        K2R_HIP(hipMemcpy(tmp.data(), stage.p, total * es, hipMemcpyDeviceToHost));
        for (size_t q = 0; q < nq; q++) {
            const uint64_t cells = cube_cells(norm_cube(cubes[q]));
            if (cells) std::memcpy((uint8_t*)out + out_offset[q] * es, tmp.data() + base[q] * es, cells * es);
        }
        return DCDF_OK;
    }
};

// ---- what k2r_query.hip defines for the raster layer.  The launchers are asynchronous on the null stream and return a DCDF code.
// the fill walk over n items; e0 / e1 (may be null) are recorded around it; synchronises the device
int launch_window_items_dev(const DevBuf& d_refs, const WinItem* d_items, uint32_t n, void* d_out, int32_t dtype, hipEvent_t e0, hipEvent_t e1,
                            bool node_wise, bool narrow);
// the node-wise search walk: the matches of item i as a bitmap of 64 rows x 2 words at d_wbits[128 * i]
int launch_search_walk(const ChunkRef* d_refs, const WinItem* d_witems, uint32_t nw, void* d_wbits, const SearchExtra* d_sx, bool narrow,
                       bool value);
int launch_search_count(const uint32_t* d_wbits, const SearchItem* d_items, const WinQuery* d_qs, uint32_t ni, uint32_t* d_counts);
int launch_search_emit(const WinQuery* d_qs, const SearchItem* d_items, uint32_t ni, const uint32_t* d_bits, const uint32_t* d_wbits,
                       const uint64_t* d_offs, uint32_t* d_out);

struct SearchCtx {  // a raster's view of its chunks (dcdf_raster_search_batch): nothing to de-duplicate or upload per call
    const DevBuf* refs;        // ChunkRef table, one entry per chunk of the raster
    const uint32_t* chunk_of;  // per query: index into it
    const uint32_t* origin;    // per query: (instant, row, col) of the chunk inside the raster, added to every triple
    bool node_wise, all_narrow;
    bool wave_ok;              // every chunk has k * k <= 64 (k_search_wave for the arities the node walk does not take)
};
// vlower / vupper (value search, lower / upper unused): real-valued bounds, translated per query with the chunk's encoding and
// fractional bits (value_bounds); the walks then run their VALUE instantiations
int search_impl(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper, size_t nq, uint32_t* out,
                size_t cap, uint64_t* counts, uint64_t* offsets, size_t* total_out, float* kernel_ms, int out_mem = DCDF_MEM_HOST,
                const SearchCtx* ctx = nullptr, const double* vlower = nullptr, const double* vupper = nullptr);

}  // namespace k2r
