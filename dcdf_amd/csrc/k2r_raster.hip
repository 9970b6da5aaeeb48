// k2r_raster.hip -- C ABI, query side: a tiled, time-segmented raster of opened chunks (dcdf_raster_*).  Routes dataset-level cubes
// and points to their chunks on the device and runs the walks of k2r_query.hip / k2r_bulk.hip over the pieces.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <new>

#include "k2r_bulk.h"
#include "k2r_decode.h"
#include "k2r_hist.h"
#include "k2r_query_host.h"
#include "k2r_reduce.h"
#include "k2r_space.h"

using namespace k2r;

// ---- a tiled, time-segmented raster of opened chunks: the routing of the layers above, natively ---------------------------------
// Variable::append cuts [instants, rows, cols] into time segments of chunk_size instants (dataset.rs:838) and Superchunk::build
// cuts each segment into tile x tile sub-arrays (superchunk.rs:127-181); reads are routed back the same way (Span::fill_window
// span.rs:190-216 over time, Superchunk::subchunks_for superchunk.rs:589-633 over rows / cols).  dcdf_raster does that split for a
// whole batch of dataset-level cubes on the host in C++ and decodes every piece in ONE launch straight into its place in the
// caller's window (the pieces carry the parent window's strides): no per-piece copies, no reassembly, the chunk table uploaded once.
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
    DevBuf d_refs;
    DevBuf d_quirk;  // [chunk][chunk_size]: dcdf_chunk::search_quirk of every instant (k_raster_search_expand)
    DevBuf d_enc;    // [chunk]: the chunk's encoding (value search translates its bounds per piece on the device)
    bool all_wave = true, all_node = true, all_narrow = true;
    bool bad_fbits = false;  // a float chunk with fractional bits value_bounds does not take (> 62)
    // tiled rasters (dcdf_raster_create_tiles): the grid is one of leaves; chunks[] / d_refs hold NULL / zeros for elided leaves
    // and the all_* flags are over chunk leaves only
    bool tiled = false;
    std::vector<RasterLeaf> leaves;  // [leaf]
    DevBuf d_leaf;                   // the same on the device
    DevBuf d_vals;                   // [leaf][chunk_size] int64: an elided leaf's value per instant (0 elsewhere)
    DevBuf d_mm;                     // [leaf][chunk_size][2] int64: the holding node's (min, max) per instant (RasterLeaf::has_mm)
};
// what dcdf_raster_create and dcdf_raster_create_tiles share: the grid, the per-leaf tables, "chunk h is leaf i", the uploads
struct RasterTables {
    std::vector<ChunkRef> refs;
    std::vector<uint8_t> quirk, enc;
};
static int raster_init(const void* leaves, size_t n, const uint32_t shape[3], uint32_t tile, uint32_t chunk_size, dcdf_raster** out,
                       std::unique_ptr<dcdf_raster>& r, RasterTables& t) {
    if (!leaves || !shape || !out || tile == 0 || chunk_size == 0 || shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    r.reset(new (std::nothrow) dcdf_raster());
    if (!r) return DCDF_ERR_NOMEM;
    r->T = shape[0]; r->R = shape[1]; r->C = shape[2]; r->tile = tile; r->cs = chunk_size;
    r->nseg = (r->T + chunk_size - 1) / chunk_size;
    r->nti = (r->R + tile - 1) / tile;
    r->ntj = (r->C + tile - 1) / tile;
    if ((uint64_t)r->nseg * r->nti * r->ntj != n) return DCDF_ERR_BAD_ARG;
    r->chunks.assign(n, nullptr);
    t.refs.assign(n, ChunkRef{});
    t.quirk.assign(n * (size_t)chunk_size, 0);
    t.enc.assign(n, 0);
    return DCDF_OK;
}
// the instants, rows and columns of leaf i
static void raster_leaf_shape(const dcdf_raster* r, size_t i, uint32_t* li, uint32_t* lr, uint32_t* lc) {
    const uint32_t seg = (uint32_t)(i / ((size_t)r->nti * r->ntj)), ti = (uint32_t)(i / r->ntj % r->nti), tj = (uint32_t)(i % r->ntj);
    *li = std::min(r->cs, r->T - seg * r->cs);
    *lr = std::min(r->tile, r->R - ti * r->tile);
    *lc = std::min(r->tile, r->C - tj * r->tile);
}
static void raster_add_chunk(dcdf_raster* r, RasterTables& t, size_t i, dcdf_chunk* h) {
    r->chunks[i] = h;
    if (h->store && (r->keep.empty() || r->keep.back() != h->store)) r->keep.push_back(h->store);
    t.refs[i] = make_ref(h);
    r->all_wave = r->all_wave && wave_kernel_ok(h);
    r->all_node = r->all_node && node_kernel_ok(h);
    r->all_narrow = r->all_narrow && h->narrow32;
    for (size_t k = 0; k < h->search_quirk.size() && k < r->cs; k++) t.quirk[i * r->cs + k] = h->search_quirk[k];
    t.enc[i] = (uint8_t)h->encoding;
    if ((h->encoding == DCDF_F32 || h->encoding == DCDF_F64) && h->fbits > 62) r->bad_fbits = true;
}
static int raster_upload(dcdf_raster* r, const RasterTables& t) {
    K2R_HIP(upload(r->d_refs, t.refs));
    K2R_HIP(upload(r->d_quirk, t.quirk));
    K2R_HIP(upload(r->d_enc, t.enc));
    return DCDF_OK;
}
extern "C" int dcdf_raster_create(dcdf_chunk* const* chunks, size_t n_chunks, const uint32_t shape[3], uint32_t tile, uint32_t chunk_size,
                                  dcdf_raster** out) {
    std::unique_ptr<dcdf_raster> r;
    RasterTables t;
    int rc = raster_init(chunks, n_chunks, shape, tile, chunk_size, out, r, t);
    if (rc != DCDF_OK) return rc;
    for (size_t i = 0; i < n_chunks; i++) {
        dcdf_chunk* h = chunks[i];
        if (!h) return DCDF_ERR_BAD_ARG;
        uint32_t li, lr, lc;
        raster_leaf_shape(r.get(), i, &li, &lr, &lc);
        // every chunk must have the shape its place in the grid gives it
        if (h->instants != li || h->rows != lr || h->cols != lc) return DCDF_ERR_BAD_ARG;
        raster_add_chunk(r.get(), t, i, h);
    }
    rc = raster_upload(r.get(), t);
    if (rc != DCDF_OK) return rc;
    *out = r.release();
    return DCDF_OK;
}
extern "C" void dcdf_raster_destroy(dcdf_raster* r) { delete r; }
// a raster over stored Superchunks (dcdf_k2r.h): the grid of leaves, each a chunk (possibly offset inside a chunk that spans
// several leaves) or an elided leaf with one value per instant
extern "C" int dcdf_raster_create_tiles(const dcdf_raster_tile* tiles, size_t n_tiles, const uint32_t shape[3], uint32_t tile,
                                        uint32_t chunk_size, dcdf_raster** out) {
    std::unique_ptr<dcdf_raster> r;
    RasterTables t;
    int rc = raster_init(tiles, n_tiles, shape, tile, chunk_size, out, r, t);
    if (rc != DCDF_OK) return rc;
    r->tiled = true;
    r->leaves.assign(n_tiles, RasterLeaf{});
    std::vector<int64_t> vals(n_tiles * (size_t)chunk_size, 0), mm(2 * n_tiles * (size_t)chunk_size, 0);
    for (size_t i = 0; i < n_tiles; i++) {
        const dcdf_raster_tile& L = tiles[i];
        uint32_t li, lr, lc;
        raster_leaf_shape(r.get(), i, &li, &lr, &lc);
        if (L.encoding != DCDF_I32 && L.encoding != DCDF_I64 && L.encoding != DCDF_F32 && L.encoding != DCDF_F64) return DCDF_ERR_BAD_ARG;
        if ((L.encoding == DCDF_F32 || L.encoding == DCDF_F64) && L.fractional_bits > 62) return DCDF_ERR_BAD_ARG;
        RasterLeaf& f = r->leaves[i];
        f.enc = L.encoding;
        f.fbits = L.fractional_bits;
        f.has_mm = L.minmax != nullptr;
        f.exact = L.minmax_exact != 0;
        if (L.minmax)
            for (uint32_t k = 0; k < li; k++) {
                mm[(i * chunk_size + k) * 2] = L.minmax[2 * k];
                mm[(i * chunk_size + k) * 2 + 1] = L.minmax[2 * k + 1];
            }
        dcdf_chunk* h = L.chunk;
        if (!h) {
            if (!L.values) return DCDF_ERR_BAD_ARG;
            f.elided = 1;
            for (uint32_t k = 0; k < li; k++) vals[i * chunk_size + k] = L.values[k];
            t.enc[i] = (uint8_t)L.encoding;
            continue;
        }
        // the chunk must cover the leaf at (row0, col0), with the leaf's instants
        if (h->instants != li || (uint64_t)L.row0 + lr > h->rows || (uint64_t)L.col0 + lc > h->cols) return DCDF_ERR_BAD_ARG;
        f.row0 = L.row0;
        f.col0 = L.col0;
        raster_add_chunk(r.get(), t, i, h);
    }
    rc = raster_upload(r.get(), t);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(upload(r->d_leaf, r->leaves));
    K2R_HIP(upload(r->d_vals, vals));
    K2R_HIP(upload(r->d_mm, mm));
    *out = r.release();
    return DCDF_OK;
}

// the pieces of one dataset-level cube: f(chunk id, local cube, raster origin of the chunk)
template <class F>
static void raster_pieces(const dcdf_raster* r, const dcdf_cube& c, F&& f) {
    for (uint32_t seg = c.start / r->cs; seg <= (c.end - 1) / r->cs; seg++)
        for (uint32_t ti = c.top / r->tile; ti <= (c.bottom - 1) / r->tile; ti++)
            for (uint32_t tj = c.left / r->tile; tj <= (c.right - 1) / r->tile; tj++) {
                const uint32_t t0 = seg * r->cs, r0 = ti * r->tile, c0 = tj * r->tile;
                const dcdf_cube l{std::max(c.start, t0) - t0, std::min(c.end, t0 + r->cs) - t0, std::max(c.top, r0) - r0,
                                  std::min(c.bottom, r0 + r->tile) - r0, std::max(c.left, c0) - c0, std::min(c.right, c0 + r->tile) - c0};
                f((uint32_t)(((uint64_t)seg * r->nti + ti) * r->ntj + tj), l, t0, r0, c0);
            }
}
// One thread per dataset-level cube: the wave items of its pieces (the loops of raster_pieces x window_items), written at
// item_base[q]; the host only counts them (a closed form per cube) -- 24 bytes per item need not cross PCIe.
struct RasterGeom {
    uint32_t T, R, C, tile, cs, nti, ntj, step;  // step: 64 (node-wise walk) or 32
};
__global__ void __launch_bounds__(256)
k_raster_expand(const dcdf_cube* __restrict__ cubes, const uint64_t* __restrict__ out_base, const uint32_t* __restrict__ item_base, uint32_t nq,
                RasterGeom g, WinItem* __restrict__ items) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    dcdf_cube c = cubes[q];
    if (c.start > c.end) { const uint32_t x = c.start; c.start = c.end; c.end = x; }  // helpers.rs:7-16 (norm_cube)
    if (c.top > c.bottom) { const uint32_t x = c.top; c.top = c.bottom; c.bottom = x; }
    if (c.left > c.right) { const uint32_t x = c.left; c.left = c.right; c.right = x; }
    const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
    if ((uint64_t)(c.end - c.start) * wr * wc == 0) return;
    WinItem* o = items + item_base[q];
    const uint64_t base = out_base[q];
    for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++)
        for (uint32_t ti = c.top / g.tile; ti <= (c.bottom - 1) / g.tile; ti++)
            for (uint32_t tj = c.left / g.tile; tj <= (c.right - 1) / g.tile; tj++) {
                const uint32_t t0 = seg * g.cs, r0 = ti * g.tile, c0 = tj * g.tile;
                const uint32_t ls = max(c.start, t0) - t0, le = min(c.end, t0 + g.cs) - t0, lt = max(c.top, r0) - r0, lb = min(c.bottom, r0 + g.tile) - r0,
                               ll = max(c.left, c0) - c0, lr = min(c.right, c0 + g.tile) - c0;
                const uint32_t cid = (seg * g.nti + ti) * g.ntj + tj;
                const uint64_t at = base + ((uint64_t)(t0 + ls - c.start) * wr + (r0 + lt - c.top)) * wc + (c0 + ll - c.left);
                const uint32_t rs = g.step == 64 ? lt : (lt & ~31u), cs0 = g.step == 64 ? ll : (ll & ~31u);
                for (uint32_t t = ls; t < le; t++)
                    for (uint32_t rr = rs; rr < lb; rr += g.step)
                        for (uint32_t cc = cs0; cc < lr; cc += g.step) {
                            WinItem it;
                            it.chunk = cid;
                            it.inst = t;
                            it.top = (uint16_t)max(rr, lt);
                            it.bottom = (uint16_t)min(rr + g.step, lb);
                            it.left = (uint16_t)max(cc, ll);
                            it.right = (uint16_t)min(cc + g.step, lr);
                            it.out_sr = (uint32_t)wc;
                            it.out_off = at + (uint64_t)(t - ls) * wr * wc + (uint64_t)(it.top - lt) * wc + (it.left - ll);
                            *o++ = it;
                        }
            }
}
// wave items of one cube (the count of the loops above)
static uint64_t raster_item_count(const dcdf_raster* r, const dcdf_cube& c, uint32_t step) {
    auto along = [&](uint32_t a, uint32_t b, uint32_t unit) {  // sum over the tiles [a, b) meets of ceil(piece / step) (from the piece's start, or the 32-grid)
        uint64_t n = 0;
        for (uint32_t t = a / unit; t <= (b - 1) / unit; t++) {
            const uint32_t lo = std::max(a, t * unit) - t * unit, hi = std::min(b, t * unit + unit) - t * unit;
            const uint32_t from = step == 64 ? lo : (lo & ~31u);
            n += (hi - from + step - 1) / step;
        }
        return n;
    };
    return (uint64_t)(c.end - c.start) * along(c.top, c.bottom, r->tile) * along(c.left, c.right, r->tile);
}

// ---- tiled rasters: fill_window -------------------------------------------------------------------------------------------
// A piece on a chunk leaf is decoded by the wave walk at (row0 + r, col0 + c) of its chunk; a piece on an elided leaf becomes a
// ConstPiece: one value per instant over a rectangle of the window, written by k_raster_fill_const in the same call.
struct ConstPiece {
    uint32_t leaf, ls, le, rows, cols, out_sr;  // leaf-local instants [ls, le), the rectangle, the window's row stride
    uint64_t out_off, out_st;                   // element of (ls, top, left) in `out`; the window's instant stride
};
// wave items along one axis of a piece [a, b) in chunk coordinates: from the piece's start (node-wise walk, step 64) or from the
// chunk's 32-grid (step 32) -- the loops of k_raster_expand / k_raster_tiled_expand
K2R_HD uint32_t axis_items(uint32_t a, uint32_t b, uint32_t step) { return (b - (step == 64 ? a : (a & ~31u)) + step - 1) / step; }
// wave items and constant pieces of one cube of a tiled raster
static void tiled_item_count(const dcdf_raster* r, const dcdf_cube& c, uint32_t step, uint64_t* n_items, uint64_t* n_const) {
    raster_pieces(r, c, [&](uint32_t cid, const dcdf_cube& l, uint32_t, uint32_t, uint32_t) {
        const RasterLeaf& f = r->leaves[cid];
        if (f.elided) {
            (*n_const)++;
            return;
        }
        *n_items += (uint64_t)(l.end - l.start) * axis_items(f.row0 + l.top, f.row0 + l.bottom, step) *
                    axis_items(f.col0 + l.left, f.col0 + l.right, step);
    });
}
// k_raster_expand for tiled rasters: one thread per cube writes the wave items of its chunk pieces (in chunk coordinates) at
// item_base[q] and its constant pieces at const_base[q]
__global__ void __launch_bounds__(256)
k_raster_tiled_expand(const dcdf_cube* __restrict__ cubes, const uint64_t* __restrict__ out_base, const uint32_t* __restrict__ item_base,
                      const uint32_t* __restrict__ const_base, uint32_t nq, RasterGeom g, const RasterLeaf* __restrict__ leaves,
                      WinItem* __restrict__ items, ConstPiece* __restrict__ consts) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    dcdf_cube c = cubes[q];
    if (c.start > c.end) { const uint32_t x = c.start; c.start = c.end; c.end = x; }
    if (c.top > c.bottom) { const uint32_t x = c.top; c.top = c.bottom; c.bottom = x; }
    if (c.left > c.right) { const uint32_t x = c.left; c.left = c.right; c.right = x; }
    const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
    if ((uint64_t)(c.end - c.start) * wr * wc == 0) return;
    WinItem* o = items + item_base[q];
    ConstPiece* k = consts + const_base[q];
    const uint64_t base = out_base[q];
    for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++)
        for (uint32_t ti = c.top / g.tile; ti <= (c.bottom - 1) / g.tile; ti++)
            for (uint32_t tj = c.left / g.tile; tj <= (c.right - 1) / g.tile; tj++) {
                const uint32_t t0 = seg * g.cs, r0 = ti * g.tile, c0 = tj * g.tile;
                const uint32_t ls = max(c.start, t0) - t0, le = min(c.end, t0 + g.cs) - t0, lt = max(c.top, r0) - r0, lb = min(c.bottom, r0 + g.tile) - r0,
                               ll = max(c.left, c0) - c0, lr = min(c.right, c0 + g.tile) - c0;
                const uint32_t cid = (seg * g.nti + ti) * g.ntj + tj;
                const uint64_t at = base + ((uint64_t)(t0 + ls - c.start) * wr + (r0 + lt - c.top)) * wc + (c0 + ll - c.left);
                const RasterLeaf f = leaves[cid];
                if (f.elided) {
                    *k++ = ConstPiece{cid, ls, le, lb - lt, lr - ll, (uint32_t)wc, at, wr * wc};
                    continue;
                }
                const uint32_t ct = f.row0 + lt, cb = f.row0 + lb, cl = f.col0 + ll, cr = f.col0 + lr;  // chunk coordinates
                const uint32_t rs = g.step == 64 ? ct : (ct & ~31u), cs0 = g.step == 64 ? cl : (cl & ~31u);
                for (uint32_t t = ls; t < le; t++)
                    for (uint32_t rr = rs; rr < cb; rr += g.step)
                        for (uint32_t cc = cs0; cc < cr; cc += g.step) {
                            WinItem it;
                            it.chunk = cid;
                            it.inst = t;
                            it.top = (uint16_t)max(rr, ct);
                            it.bottom = (uint16_t)min(rr + g.step, cb);
                            it.left = (uint16_t)max(cc, cl);
                            it.right = (uint16_t)min(cc + g.step, cr);
                            it.out_sr = (uint32_t)wc;
                            it.out_off = at + (uint64_t)(t - ls) * wr * wc + (uint64_t)(it.top - ct) * wc + (it.left - cl);
                            *o++ = it;
                        }
            }
}
// the constant pieces: one workgroup per piece.  The value of each instant is converted once (LDS), then every 16-byte aligned
// block of a destination row is written with one 16-byte store when the row covers it whole, element by element at the ends.
constexpr uint32_t kConstBatch = 256;  // instants converted per round
__global__ void __launch_bounds__(256)
k_raster_fill_const(const ConstPiece* __restrict__ ps, uint32_t n, const RasterLeaf* __restrict__ leaves, const int64_t* __restrict__ vals,
                    uint32_t cs, void* __restrict__ out, int32_t dtype) {
    __shared__ uint64_t conv[kConstBatch];
    const uint32_t es = (dtype == ENC_I32 || dtype == ENC_F32) ? 4u : 8u;
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const ConstPiece P = ps[p];
        const uint32_t fbits = leaves[P.leaf].fbits;
        const uint32_t units = (P.cols * es + 15u) / 16u + 1u;  // aligned 16-byte blocks a row can meet
        for (uint32_t tb = P.ls; tb < P.le; tb += kConstBatch) {
            const uint32_t nt = min(kConstBatch, P.le - tb);
            __syncthreads();
            if (threadIdx.x < nt) {
                uint64_t w = 0;
                store_typed(&w, 0, dtype, vals[(uint64_t)P.leaf * cs + tb + threadIdx.x], fbits);
                conv[threadIdx.x] = w;
            }
            __syncthreads();
            const uint64_t total = (uint64_t)nt * P.rows * units;
            for (uint64_t e = threadIdx.x; e < total; e += blockDim.x) {
                const uint32_t u = (uint32_t)(e % units), rr = (uint32_t)(e / units % P.rows), t = (uint32_t)(e / ((uint64_t)units * P.rows));
                const uint64_t w = conv[t];
                uint8_t* const row = (uint8_t*)out + (P.out_off + (uint64_t)(tb - P.ls + t) * P.out_st + (uint64_t)rr * P.out_sr) * es;
                const uintptr_t a0 = (uintptr_t)row, a1 = a0 + (uintptr_t)P.cols * es, b0 = (a0 & ~(uintptr_t)15) + 16u * u;
                if (b0 >= a1) continue;
                if (b0 >= a0 && b0 + 16 <= a1) {
                    uint4 v;
                    if (es == 4) v = make_uint4((uint32_t)w, (uint32_t)w, (uint32_t)w, (uint32_t)w);
                    else v = make_uint4((uint32_t)w, (uint32_t)(w >> 32), (uint32_t)w, (uint32_t)(w >> 32));
                    *(uint4*)b0 = v;
                } else {
                    for (uintptr_t a = b0 > a0 ? b0 : a0; a < b0 + 16 && a < a1; a += es) {
                        if (es == 4) *(uint32_t*)a = (uint32_t)w;
                        else *(uint64_t*)a = w;
                    }
                }
            }
        }
    }
}

extern "C" int dcdf_raster_fill_window_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype,
                                             int out_mem, const uint64_t* out_offset, float* kernel_ms) {
    if (!r || !cubes || !out || !out_offset || nq == 0 || nq > 0x7fffffffu || !out_args_ok(out_dtype, out_mem)) return DCDF_ERR_BAD_ARG;
    if (!r->all_wave) return DCDF_ERR_UNSUPPORTED;  // arities beyond the wave walk (k * k > 64): use the per-chunk entry points
    const uint32_t step = r->all_node ? 64u : 32u;
    // host: bounds, where each window goes, how many wave items it makes; device: the items themselves (k_raster_expand)
    WindowOut W(cubes, nq, out, out_offset, elem_size(out_dtype), out_mem == DCDF_MEM_DEVICE);
    std::vector<uint32_t> item_base(nq), const_base(r->tiled ? nq : 0);
    uint64_t n_items = 0, n_const = 0;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
        const uint64_t cells = cube_cells(c);
        item_base[q] = (uint32_t)n_items;
        if (r->tiled) {
            const_base[q] = (uint32_t)n_const;
            if (cells) tiled_item_count(r, c, step, &n_items, &n_const);
            if (n_const > 0xfffffff0ull) return DCDF_ERR_CAPACITY;
        } else if (cells) {
            n_items += raster_item_count(r, c, step);
        }
        if (n_items > 0xfffffff0ull) return DCDF_ERR_CAPACITY;
    }
    if (n_items == 0 && n_const == 0) return DCDF_OK;
    DevBuf d_cubes, d_base, d_ibase, d_items, d_cbase, d_consts;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    K2R_HIP(upload(d_cubes, cubes, nq * sizeof(dcdf_cube)));
    K2R_HIP(upload(d_base, W.base));
    K2R_HIP(upload(d_ibase, item_base));
    K2R_HIP(d_items.alloc_pooled(n_items * sizeof(WinItem)));
    const RasterGeom g{r->T, r->R, r->C, r->tile, r->cs, r->nti, r->ntj, step};
    EventPair ev;
    K2R_HIP(ev.create());
    int rc = DCDF_OK;
    if (!r->tiled) {
        hipLaunchKernelGGL(k_raster_expand, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, 0, d_cubes.as<dcdf_cube>(), d_base.as<uint64_t>(),
                           d_ibase.as<uint32_t>(), (uint32_t)nq, g, d_items.as<WinItem>());
        K2R_HIP(hipGetLastError());
        rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>(), (uint32_t)n_items, W.dst(), out_dtype, ev.e0, ev.e1, r->all_node, r->all_narrow);
    } else {  // chunk pieces as above, elided pieces filled by k_raster_fill_const; the time covers both
        K2R_HIP(upload(d_cbase, const_base));
        K2R_HIP(d_consts.alloc_pooled(n_const * sizeof(ConstPiece)));
        hipLaunchKernelGGL(k_raster_tiled_expand, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, 0, d_cubes.as<dcdf_cube>(), d_base.as<uint64_t>(),
                           d_ibase.as<uint32_t>(), d_cbase.as<uint32_t>(), (uint32_t)nq, g, r->d_leaf.as<RasterLeaf>(), d_items.as<WinItem>(),
                           d_consts.as<ConstPiece>());
        K2R_HIP(hipGetLastError());
        K2R_HIP(hipEventRecord(ev.e0, 0));
        if (n_const)
            hipLaunchKernelGGL(k_raster_fill_const, dim3((uint32_t)std::min<uint64_t>(n_const, 256u * 64u)), dim3(256), 0, 0, d_consts.as<ConstPiece>(),
                               (uint32_t)n_const, r->d_leaf.as<RasterLeaf>(), r->d_vals.as<int64_t>(), r->cs, W.dst(), out_dtype);
        K2R_HIP(hipGetLastError());
        if (n_items) {
            rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>(), (uint32_t)n_items, W.dst(), out_dtype, nullptr, ev.e1, r->all_node,
                                         r->all_narrow);
        } else {
            K2R_HIP(hipEventRecord(ev.e1, 0));
            K2R_HIP(hipDeviceSynchronize());
        }
    }
    if (rc == DCDF_OK) rc = W.finish();
    if (rc != DCDF_OK) return rc;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
// ---- decompress: whole regions, block by block (k2r_bulk.hip) ---------------------------------------------------------------
// The pieces of every cube, by the kind of leaf they fall on: a chunk with a side-16 table and 32-bit values becomes BulkUnits (a
// workgroup per 64 x 64 region of the chunk's grid, looping over the piece's instants); any other chunk the wave items
// dcdf_raster_fill_window_batch makes of it; an elided leaf a ConstPiece.  All three write the same output array.
extern "C" int dcdf_raster_decode_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype, int out_mem,
                                        const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    if (!r || !cubes || !out || !out_offset || nq > 0x7fffffffu || !out_args_ok(out_dtype, out_mem)) return DCDF_ERR_BAD_ARG;
    if (!r->all_wave) return DCDF_ERR_UNSUPPORTED;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (kernel_ms) *kernel_ms = 0.f;
    if (nq == 0) return DCDF_OK;
    WindowOut W(cubes, nq, out, out_offset, elem_size(out_dtype), out_mem == DCDF_MEM_DEVICE);
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
    }
    std::vector<BulkUnit> units;
    std::vector<WinItem> items;
    std::vector<ConstPiece> consts;
    uint64_t n_bulk = 0, n_walk = 0, n_const = 0;  // cells
    uint32_t max_nt = 0;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if ((uint64_t)(c.end - c.start) * wr * wc == 0) continue;
        raster_pieces(r, c, [&](uint32_t cid, const dcdf_cube& l, uint32_t t0, uint32_t r0, uint32_t c0) {
            const uint64_t at = W.base[q] + ((uint64_t)(t0 + l.start - c.start) * wr + (r0 + l.top - c.top)) * wc + (c0 + l.left - c.left);
            const uint64_t cells = cube_cells(l);
            const RasterLeaf f = r->tiled ? r->leaves[cid] : RasterLeaf{};
            if (f.elided) {
                consts.push_back(ConstPiece{cid, l.start, l.end, l.bottom - l.top, l.right - l.left, (uint32_t)wc, at, wr * wc});
                n_const += cells;
                return;
            }
            const dcdf_chunk* h = r->chunks[cid];
            const dcdf_cube k{l.start, l.end, f.row0 + l.top, f.row0 + l.bottom, f.col0 + l.left, f.col0 + l.right};  // chunk coordinates
            if (!(h->top_g && h->narrow32)) {
                window_items(cid, k, at, items, r->all_node, wc, wr * wc);
                n_walk += cells;
                return;
            }
            for (uint32_t rr = k.top & ~(BULK_REGION - 1); rr < k.bottom; rr += BULK_REGION)
                for (uint32_t rc = k.left & ~(BULK_REGION - 1); rc < k.right; rc += BULK_REGION) {
                    BulkUnit u{};
                    u.chunk = cid;
                    u.t0 = k.start;
                    u.t1 = k.end;
                    u.rr = (uint16_t)rr;
                    u.rc = (uint16_t)rc;
                    u.top = (uint16_t)std::max(rr, k.top);
                    u.bottom = (uint16_t)std::min(rr + BULK_REGION, k.bottom);
                    u.left = (uint16_t)std::max(rc, k.left);
                    u.right = (uint16_t)std::min(rc + BULK_REGION, k.right);
                    u.out_sr = (uint32_t)wc;
                    u.out_st = wr * wc;
                    u.out_off = at + (uint64_t)(u.top - k.top) * wc + (u.left - k.left);
                    units.push_back(u);
                }
            max_nt = std::max(max_nt, k.end - k.start);
            n_bulk += cells;
        });
        if (units.size() > 0x3fffffffull || items.size() > 0xfffffff0ull || consts.size() > 0xfffffff0ull) return DCDF_ERR_CAPACITY;
    }
    if (stats) {
        stats[0] = n_bulk;
        stats[1] = n_walk;
        stats[2] = n_const;
    }
    if (W.total == 0) return DCDF_OK;
    // few units: a unit's instants in several workgroups (bulk_parts; each decodes its Snapshot again)
    const uint32_t parts = bulk_parts(units.size(), max_nt, bulk_wanted_units());
    if (parts > 1) {
        std::vector<BulkUnit> split;
        split.reserve(units.size() * parts);
        for (const BulkUnit& u : units) {
            const uint32_t nt = u.t1 - u.t0, np = bulk_parts(units.size(), nt, bulk_wanted_units());
            for (uint32_t j = 0; j < np; j++) {
                BulkUnit v = u;
                v.t0 = bulk_part(u.t0, nt, np, j);
                v.t1 = bulk_part(u.t0, nt, np, j + 1);
                v.out_off = u.out_off + (uint64_t)(v.t0 - u.t0) * u.out_st;
                if (v.t1 > v.t0) split.push_back(v);
            }
        }
        units.swap(split);
    }
    DevBuf d_units, d_consts;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    void* const d_out = W.dst();
    if (!units.empty()) {
        K2R_HIP(d_units.alloc_pooled(units.size() * sizeof(BulkUnit)));
        K2R_HIP(hipMemcpy(d_units.p, units.data(), units.size() * sizeof(BulkUnit), hipMemcpyHostToDevice));
    }
    if (!consts.empty()) {
        K2R_HIP(d_consts.alloc_pooled(consts.size() * sizeof(ConstPiece)));
        K2R_HIP(hipMemcpy(d_consts.p, consts.data(), consts.size() * sizeof(ConstPiece), hipMemcpyHostToDevice));
    }
    DevBuf d_items;
    if (!items.empty()) {
        K2R_HIP(d_items.alloc_pooled(items.size() * sizeof(WinItem)));
        K2R_HIP(hipMemcpy(d_items.p, items.data(), items.size() * sizeof(WinItem), hipMemcpyHostToDevice));
    }
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    if (!consts.empty()) {
        hipLaunchKernelGGL(k_raster_fill_const, dim3((uint32_t)std::min<uint64_t>(consts.size(), 256u * 64u)), dim3(256), 0, 0, d_consts.as<ConstPiece>(),
                           (uint32_t)consts.size(), r->d_leaf.as<RasterLeaf>(), r->d_vals.as<int64_t>(), r->cs, d_out, out_dtype);
        K2R_HIP(hipGetLastError());
    }
    const int rcb = launch_bulk_decode(r->d_refs.as<ChunkRef>(), d_units.as<BulkUnit>(), (uint32_t)units.size(), d_out, out_dtype);
    if (rcb != DCDF_OK) return rcb;
    if (!items.empty()) {
        const int rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>(), (uint32_t)items.size(), d_out, out_dtype, nullptr, ev.e1, r->all_node,
                                               r->all_narrow);
        if (rc != DCDF_OK) return rc;
    } else {
        K2R_HIP(hipEventRecord(ev.e1, 0));
        K2R_HIP(hipDeviceSynchronize());
    }
    const int rcf = W.finish();
    if (rcf != DCDF_OK) return rcf;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
// ---- reduce over time: per-cell min / max / sum / count / mean of the values decode returns (k2r_reduce.h) --------------------
// The pieces of every cube are classified as dcdf_raster_decode_batch classifies them.  What keeps the sum's order: within a
// time segment every cell of a cube lies in exactly one piece (raster_pieces), so the work of one segment never shares a cell;
// the segments are launched one after the other, in ascending order, on the null stream, and each piece continues the running
// sum its cells' state plane holds.  The state planes are the output planes themselves (cube q's requested planes in ascending
// bit order); SUM / COUNT kept for MEAN alone live in scratch planes.
//
// Pieces on chunks the bulk kernel does not take are decoded by the window walk as stored integers (DCDF_I64: store_typed
// leaves n as it is) into a slab of a bounded number of cells, then folded by k_reduce_fold, which applies the leaf's own
// encoding (reduce_widen: the conversions of store_typed, so the value is the typed fill_window's) -- one walk launch per slab
// whatever mix of encodings its chunks have.  Elided pieces are folded by the same kernel straight from dcdf_raster::d_vals.
__global__ void __launch_bounds__(256)
k_reduce_fold(const FoldPiece* __restrict__ ps, uint32_t n, const int64_t* __restrict__ slab, const int64_t* __restrict__ vals, double* dst,
              double* scr, uint32_t ops) {
    const uint32_t live = reduce_live(ops);
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const FoldPiece P = ps[p];
        const uint64_t cells = (uint64_t)P.rows * P.cols;
        double* const p_min = reduce_plane(RA_MIN, dst, scr, ops, P.o_off, P.s_off, P.psz);
        double* const p_max = reduce_plane(RA_MAX, dst, scr, ops, P.o_off, P.s_off, P.psz);
        double* const p_sum = reduce_plane(RA_SUM, dst, scr, ops, P.o_off, P.s_off, P.psz);
        double* const p_cnt = reduce_plane(RA_COUNT, dst, scr, ops, P.o_off, P.s_off, P.psz);
        for (uint64_t e = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; e < cells; e += (uint64_t)gridDim.y * blockDim.x) {
            const uint64_t at = e / P.cols * P.sr + e % P.cols;
            double s = 0.0, c = 0.0, lo = __builtin_nan(""), hi = __builtin_nan("");
            if (!P.init) {
                if (live & RA_MIN) lo = p_min[at];
                if (live & RA_MAX) hi = p_max[at];
                if (live & RA_SUM) s = p_sum[at];
                if (live & RA_COUNT) c = p_cnt[at];
            }
            for (uint32_t t = 0; t < P.nt; t++) {
                const double x = reduce_widen(P.enc, P.fbits, P.elided ? vals[P.src + t] : slab[P.src + (uint64_t)t * cells + e]);
                if (x == x) {
                    s = s + x;
                    c = c + 1.0;
                    lo = fmin(lo, x);
                    hi = fmax(hi, x);
                }
            }
            if (live & RA_MIN) p_min[at] = lo;
            if (live & RA_MAX) p_max[at] = hi;
            if (live & RA_SUM) p_sum[at] = s;
            if (live & RA_COUNT) p_cnt[at] = c;
        }
    }
}
// the finishing kernel: MEAN = SUM / COUNT, NaN where nothing was counted
__global__ void __launch_bounds__(256) k_reduce_mean(const MeanPiece* __restrict__ ps, uint32_t n, double* dst, double* scr, uint32_t ops) {
    for (uint32_t p = blockIdx.y; p < n; p += gridDim.y) {
        const MeanPiece P = ps[p];
        const double* const p_sum = reduce_plane(RA_SUM, dst, scr, ops, P.o_off, P.s_off, P.psz);
        const double* const p_cnt = reduce_plane(RA_COUNT, dst, scr, ops, P.o_off, P.s_off, P.psz);
        double* const p_mean = dst + P.o_off + (uint64_t)popc32(ops & RA_ALL) * P.psz;
        for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < P.psz; e += (uint64_t)gridDim.x * blockDim.x) {
            const double c = p_cnt[e];
            p_mean[e] = c == 0.0 ? __builtin_nan("") : p_sum[e] / c;
        }
    }
}
// cells of one fallback slab (K2R_REDUCE_SLAB_CELLS overrides: tests of the slab cut)
static uint64_t reduce_slab_cells() {
    const char* e = std::getenv("K2R_REDUCE_SLAB_CELLS");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : (uint64_t)1 << 22;
}
static int launch_reduce_fold(const FoldPiece* d_ps, uint32_t n, const int64_t* d_slab, const int64_t* d_vals, double* d_dst, double* d_scr,
                              uint32_t ops) {
    if (n == 0) return DCDF_OK;
    hipLaunchKernelGGL(k_reduce_fold, dim3(std::min<uint32_t>(n, 1u << 20), 16), dim3(256), 0, 0, d_ps, n, d_slab, d_vals, d_dst, d_scr, ops);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}
extern "C" int dcdf_raster_reduce_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, double* out, int out_mem,
                                             const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    if (!r || !cubes || !out || !out_offset || nq > 0x7fffffffu || ops == 0 || ops > (RA_ALL | ROP_MEAN) ||
        (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE))
        return DCDF_ERR_BAD_ARG;
    if (!r->all_wave) return DCDF_ERR_UNSUPPORTED;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (kernel_ms) *kernel_ms = 0.f;
    if (nq == 0) return DCDF_OK;
    const uint32_t live = reduce_live(ops), n_out = popc32(ops), n_scr = popc32(live & ~ops);
    // where the planes go: cube q's are n_out "instants" of [rows][cols] to WindowOut
    std::vector<dcdf_cube> planes(nq, dcdf_cube{});
    std::vector<uint64_t> sbase(nq, 0);
    uint64_t scr_total = 0;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
        if (cube_cells(c) == 0) continue;
        planes[q] = dcdf_cube{0, n_out, c.top, c.bottom, c.left, c.right};
        sbase[q] = scr_total;
        scr_total += (uint64_t)n_scr * (c.bottom - c.top) * (c.right - c.left);
    }
    WindowOut W(planes.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    // the plan, segment by segment
    struct WalkPiece {  // a piece for the window walk: chunk, chunk-level cube, and its fold without the slab offset
        uint32_t chunk;
        dcdf_cube k;
        FoldPiece f;
    };
    struct Segment {
        std::vector<ReduceUnit> units;
        std::vector<FoldPiece> consts;
        std::vector<WalkPiece> walks;
    };
    std::vector<Segment> segs(r->nseg);
    std::vector<MeanPiece> means;
    uint64_t n_bulk = 0, n_walk = 0, n_const = 0;  // cells read
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if ((uint64_t)(c.end - c.start) * wr * wc == 0) continue;
        means.push_back(MeanPiece{W.base[q], sbase[q], wr * wc});
        raster_pieces(r, c, [&](uint32_t cid, const dcdf_cube& l, uint32_t t0, uint32_t r0, uint32_t c0) {
            Segment& S = segs[t0 / r->cs];
            const uint64_t in_plane = (uint64_t)(r0 + l.top - c.top) * wc + (c0 + l.left - c.left);
            const uint32_t init = t0 + l.start == c.start;
            const uint64_t cells = cube_cells(l);
            const RasterLeaf f = r->tiled ? r->leaves[cid] : RasterLeaf{};
            FoldPiece p{l.end - l.start, l.bottom - l.top, l.right - l.left, (uint32_t)wc, init, f.enc, f.fbits, 1u,
                        (uint64_t)cid * r->cs + l.start, W.base[q] + in_plane, sbase[q] + in_plane, wr * wc};
            if (f.elided) {
                S.consts.push_back(p);
                n_const += cells;
                return;
            }
            const dcdf_chunk* h = r->chunks[cid];
            const dcdf_cube k{l.start, l.end, f.row0 + l.top, f.row0 + l.bottom, f.col0 + l.left, f.col0 + l.right};  // chunk coordinates
            if (!(h->top_g && h->narrow32)) {
                p.enc = h->encoding;
                p.fbits = h->fbits;
                p.elided = 0;
                S.walks.push_back(WalkPiece{cid, k, p});
                n_walk += cells;
                return;
            }
            for (uint32_t rr = k.top & ~(BULK_REGION - 1); rr < k.bottom; rr += BULK_REGION)
                for (uint32_t rc = k.left & ~(BULK_REGION - 1); rc < k.right; rc += BULK_REGION) {
                    ReduceUnit u{};
                    u.chunk = cid;
                    u.t0 = k.start;
                    u.t1 = k.end;
                    u.rr = (uint16_t)rr;
                    u.rc = (uint16_t)rc;
                    u.top = (uint16_t)std::max(rr, k.top);
                    u.bottom = (uint16_t)std::min(rr + BULK_REGION, k.bottom);
                    u.left = (uint16_t)std::max(rc, k.left);
                    u.right = (uint16_t)std::min(rc + BULK_REGION, k.right);
                    u.sr = (uint32_t)wc;
                    u.init = init;
                    const uint64_t in_piece = (uint64_t)(u.top - k.top) * wc + (u.left - k.left);
                    u.o_off = p.o_off + in_piece;
                    u.s_off = p.s_off + in_piece;
                    u.psz = wr * wc;
                    S.units.push_back(u);
                }
            n_bulk += cells;
        });
    }
    if (stats) {
        stats[0] = n_bulk;
        stats[1] = n_walk;
        stats[2] = n_const;
    }
    if (W.total == 0) return DCDF_OK;
    // One upload of every segment's work.  The window walk's pieces are cut into slabs here: a slab holds whole pieces up to the
    // cell bound; a piece beyond it is cut in time, each part a slab of its own (two parts of one piece share their cells, so
    // they must not be folded by the same launch).
    struct Slab {
        size_t item0, item1, fold0, fold1;
    };
    struct SegRange {
        size_t unit0, unit1, const0, const1, slab0, slab1;
    };
    std::vector<ReduceUnit> units;
    std::vector<FoldPiece> folds;
    std::vector<WinItem> items;
    std::vector<Slab> slabs;
    std::vector<SegRange> ranges;
    const uint64_t slab_cap = reduce_slab_cells();
    uint64_t slab_max = 0;
    for (Segment& S : segs) {
        if (S.units.empty() && S.consts.empty() && S.walks.empty()) continue;
        SegRange g{units.size(), 0, folds.size(), 0, slabs.size(), 0};
        units.insert(units.end(), S.units.begin(), S.units.end());
        folds.insert(folds.end(), S.consts.begin(), S.consts.end());
        g.unit1 = units.size();
        g.const1 = folds.size();
        Slab cur{items.size(), 0, folds.size(), 0};
        uint64_t used = 0;
        auto flush = [&] {
            cur.item1 = items.size();
            cur.fold1 = folds.size();
            if (cur.fold1 > cur.fold0) slabs.push_back(cur);
            slab_max = std::max(slab_max, used);
            cur = Slab{items.size(), 0, folds.size(), 0};
            used = 0;
        };
        for (const WalkPiece& w : S.walks) {
            const uint64_t plane = (uint64_t)w.f.rows * w.f.cols;
            const uint32_t nt = w.f.nt, step = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, slab_cap / plane));
            if (step < nt || used + (uint64_t)nt * plane > slab_cap) flush();
            for (uint32_t a = 0; a < nt; a += step) {
                const uint32_t b = std::min(nt, a + step);
                dcdf_cube k = w.k;
                k.start = w.k.start + a;
                k.end = w.k.start + b;
                FoldPiece f = w.f;
                f.nt = b - a;
                f.init = w.f.init && a == 0;
                f.src = used;
                window_items(w.chunk, k, used, items, r->all_node);
                folds.push_back(f);
                used += (uint64_t)(b - a) * plane;
                if (step < nt) flush();
            }
        }
        flush();
        g.slab1 = slabs.size();
        ranges.push_back(g);
        S = Segment{};
        if (units.size() > 0x3fffffffull || items.size() > 0xfffffff0ull || folds.size() > 0xfffffff0ull) return DCDF_ERR_CAPACITY;
    }
    DevBuf d_units, d_folds, d_items, d_means, d_slab, d_scr;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    double* const d_dst = (double*)W.dst();
    if (scr_total) K2R_HIP(d_scr.alloc_pooled(scr_total * sizeof(double)));
    if (!units.empty()) K2R_HIP(upload(d_units, units));
    if (!folds.empty()) K2R_HIP(upload(d_folds, folds));
    if (!items.empty()) K2R_HIP(upload(d_items, items));
    if (slab_max) K2R_HIP(d_slab.alloc_pooled(slab_max * sizeof(int64_t)));
    if (ops & ROP_MEAN) K2R_HIP(upload(d_means, means));
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    for (const SegRange& g : ranges) {
        int rc = launch_reduce_fold(d_folds.as<FoldPiece>() + g.const0, (uint32_t)(g.const1 - g.const0), nullptr, r->d_vals.as<int64_t>(), d_dst,
                                    d_scr.as<double>(), ops);
        if (rc != DCDF_OK) return rc;
        rc = launch_bulk_reduce(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), d_units.as<ReduceUnit>() + g.unit0, (uint32_t)(g.unit1 - g.unit0),
                                d_dst, d_scr.as<double>(), ops);
        if (rc != DCDF_OK) return rc;
        for (size_t s = g.slab0; s < g.slab1; s++) {
            const Slab& b = slabs[s];
            rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>() + b.item0, (uint32_t)(b.item1 - b.item0), d_slab.p, DCDF_I64, nullptr,
                                         nullptr, r->all_node, r->all_narrow);
            if (rc != DCDF_OK) return rc;
            rc = launch_reduce_fold(d_folds.as<FoldPiece>() + b.fold0, (uint32_t)(b.fold1 - b.fold0), d_slab.as<int64_t>(), nullptr, d_dst,
                                    d_scr.as<double>(), ops);
            if (rc != DCDF_OK) return rc;
        }
    }
    if (ops & ROP_MEAN) {
        uint64_t big = 0;
        for (const MeanPiece& m : means) big = std::max(big, m.psz);
        hipLaunchKernelGGL(k_reduce_mean, dim3((uint32_t)std::min<uint64_t>((big + 255) / 256, 2048), (uint32_t)std::min<size_t>(means.size(), 65535)),
                           dim3(256), 0, 0, d_means.as<MeanPiece>(), (uint32_t)means.size(), d_dst, d_scr.as<double>(), ops);
        K2R_HIP(hipGetLastError());
    }
    K2R_HIP(hipEventRecord(ev.e1, 0));
    K2R_HIP(hipDeviceSynchronize());
    const int rcf = W.finish();
    if (rcf != DCDF_OK) return rcf;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
// ---- reduce over space: per-instant min / max / sum / count / mean of the selected cells of a cube (k2r_space.h) ------------
// The pieces of every cube are classified as dcdf_raster_decode_batch classifies them.  Every piece -- a 64 x 64 unit of the bulk
// kernel, a piece of the window walk, an elided piece -- leaves one SpacePartial per instant in a pooled scratch array; the
// pieces of one (cube, segment) share their instants, so their records form one block [slot][instant] that k_space_finish folds
// into the cube's series.  Instants are independent: one launch of each kind takes the work of all segments and cubes.
//
// 128-bit sums and the extremes of one wave's lanes into lane 0 .. and of a workgroup's four waves into thread 0 (LDS)
struct SpaceAcc {
    uint64_t hi, lo;
    double mn, mx;
    uint32_t cnt;
};
__device__ __forceinline__ void space_block_fold(SpaceAcc& a, SpaceAcc* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t bh = (uint64_t)__shfl_xor((unsigned long long)a.hi, off), bl = (uint64_t)__shfl_xor((unsigned long long)a.lo, off);
        space_add128(a.hi, a.lo, bh, bl);
        a.cnt += __shfl_xor(a.cnt, off);
        a.mn = fmin(a.mn, __shfl_xor(a.mn, off));
        a.mx = fmax(a.mx, __shfl_xor(a.mx, off));
    }
    __syncthreads();  // (the previous round's reader is done)
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < 4u; w++) {
            space_add128(a.hi, a.lo, sh[w].hi, sh[w].lo);
            a.cnt += sh[w].cnt;
            a.mn = fmin(a.mn, sh[w].mn);
            a.mx = fmax(a.mx, sh[w].mx);
        }
}
__device__ __forceinline__ void space_store(SpacePartial* recs, uint64_t at, const SpaceAcc& a, uint32_t scale) {
    __attribute__((address_space(1))) SpacePartial* const o = (__attribute__((address_space(1))) SpacePartial*)recs + at;
    o->hi = a.hi;
    o->lo = a.lo;
    o->mn = a.mn;
    o->mx = a.mx;
    o->cnt = a.cnt;
    o->scale = scale;
}
// A workgroup per (piece, instant) of the window walk's slab: the cells' stored integers widened by the leaf's own encoding,
// masked cells skipped.  An elided piece (blockIdx.y == 0 alone): its selected cells are counted once, then a thread per instant
// writes value x count.
__global__ void __launch_bounds__(256)
k_space_fold(const SpaceFold* __restrict__ ps, uint32_t n, const int64_t* __restrict__ slab, const int64_t* __restrict__ vals,
             const uint8_t* __restrict__ mask, SpacePartial* __restrict__ recs) {
    __shared__ SpaceAcc sh[4];
    __shared__ uint32_t sh_sel;
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const SpaceFold P = ps[p];
        const uint64_t cells = (uint64_t)P.rows * P.cols;
        const uint32_t scale = space_scale(P.enc, P.fbits);
        if (P.elided) {
            if (blockIdx.y != 0) continue;
            SpaceAcc a{0, 0, __builtin_nan(""), __builtin_nan(""), 0};
            if (mask) {
                for (uint64_t e = threadIdx.x; e < cells; e += blockDim.x) a.cnt += mask[P.m_off + e / P.cols * P.m_sr + e % P.cols] != 0 ? 1u : 0u;
            } else if (threadIdx.x == 0) {
                a.cnt = (uint32_t)cells;
            }
            space_block_fold(a, sh);
            if (threadIdx.x == 0) sh_sel = a.cnt;
            __syncthreads();
            const uint32_t selected = sh_sel;
            for (uint32_t t = threadIdx.x; t < P.nt; t += blockDim.x) {
                const int64_t v = vals[P.src + t];
                const double x = reduce_widen(P.enc, P.fbits, v);
                SpaceAcc o{0, 0, __builtin_nan(""), __builtin_nan(""), 0};
                if (x == x && selected) {
                    space_mul_m(o.hi, o.lo, space_m(P.enc, v), selected);
                    o.cnt = selected;
                    o.mn = o.mx = x;
                }
                space_store(recs, P.rec + t, o, scale);
            }
            continue;
        }
        for (uint32_t t = blockIdx.y; t < P.nt; t += gridDim.y) {
            SpaceAcc a{0, 0, __builtin_nan(""), __builtin_nan(""), 0};
            for (uint64_t e = threadIdx.x; e < cells; e += blockDim.x) {
                if (mask && mask[P.m_off + e / P.cols * P.m_sr + e % P.cols] == 0) continue;
                const int64_t v = slab[P.src + (uint64_t)t * cells + e];
                const double x = reduce_widen(P.enc, P.fbits, v);
                if (x == x) {
                    space_add_m(a.hi, a.lo, space_m(P.enc, v));
                    a.cnt += 1u;
                    a.mn = fmin(a.mn, x);
                    a.mx = fmax(a.mx, x);
                }
            }
            space_block_fold(a, sh);
            if (threadIdx.x == 0) space_store(recs, P.rec + t, a, scale);
        }
    }
}
// A workgroup per (job, instant): the records of the pieces that cover the instant, their sums at the common 2^-63 scale added
// in 192 bits, then the requested series -- SUM by one conversion of that integer, MEAN by one division.
__global__ void __launch_bounds__(256)
k_space_finish(const SpaceJob* __restrict__ jobs, uint32_t n, const SpacePartial* __restrict__ recs, double* dst, uint32_t ops) {
    __shared__ U192 sh_s[4];
    __shared__ uint64_t sh_c[4];
    __shared__ double sh_mn[4], sh_mx[4];
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        const SpaceJob J = jobs[j];
        for (uint32_t t = blockIdx.y; t < J.nt; t += gridDim.y) {
            U192 acc{0, 0, 0};
            uint64_t cnt = 0;
            double mn = __builtin_nan(""), mx = __builtin_nan("");
            for (uint32_t s = threadIdx.x; s < J.n_slots; s += blockDim.x) {
                const __attribute__((address_space(1))) SpacePartial* const R =
                    (const __attribute__((address_space(1))) SpacePartial*)recs + (J.rec + (uint64_t)s * J.nt + t);
                u192_add(acc, space_scaled(R->hi, R->lo, R->scale));
                cnt += R->cnt;
                mn = fmin(mn, R->mn);
                mx = fmax(mx, R->mx);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                U192 b;
                b.w0 = (uint64_t)__shfl_xor((unsigned long long)acc.w0, off);
                b.w1 = (uint64_t)__shfl_xor((unsigned long long)acc.w1, off);
                b.w2 = (uint64_t)__shfl_xor((unsigned long long)acc.w2, off);
                u192_add(acc, b);
                cnt += (uint64_t)__shfl_xor((unsigned long long)cnt, off);
                mn = fmin(mn, __shfl_xor(mn, off));
                mx = fmax(mx, __shfl_xor(mx, off));
            }
            __syncthreads();  // (the previous round's reader is done)
            if ((threadIdx.x & 63u) == 0) {
                sh_s[threadIdx.x >> 6] = acc;
                sh_c[threadIdx.x >> 6] = cnt;
                sh_mn[threadIdx.x >> 6] = mn;
                sh_mx[threadIdx.x >> 6] = mx;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (uint32_t w = 1; w < 4u; w++) {
                    u192_add(acc, sh_s[w]);
                    cnt += sh_c[w];
                    mn = fmin(mn, sh_mn[w]);
                    mx = fmax(mx, sh_mx[w]);
                }
                const double sum = space_round(acc);
                __attribute__((address_space(1))) double* o = (__attribute__((address_space(1))) double*)dst + (J.o_off + t);
                if (ops & RA_MIN) { *o = mn == mn ? mn : __builtin_nan(""); o += J.o_stride; }
                if (ops & RA_MAX) { *o = mx == mx ? mx : __builtin_nan(""); o += J.o_stride; }
                if (ops & RA_SUM) { *o = sum; o += J.o_stride; }
                if (ops & RA_COUNT) { *o = (double)cnt; o += J.o_stride; }
                if (ops & ROP_MEAN) *o = cnt == 0 ? __builtin_nan("") : sum / (double)cnt;
            }
        }
    }
}
// records of one batch of the plan (K2R_SPACE_RECORDS overrides: tests of the batch cut); 40 bytes each
static uint64_t space_record_cap() {
    const char* e = std::getenv("K2R_SPACE_RECORDS");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : (uint64_t)6 << 20;
}
extern "C" int dcdf_space_fold_records(const uint64_t* hi, const uint64_t* lo, const uint32_t* scale, size_t n, double* sum) {
    if ((n && (!hi || !lo || !scale)) || !sum) return DCDF_ERR_BAD_ARG;
    U192 acc{0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        if ((scale[i] & 255u) > 63u || scale[i] > (SPACE_NEG | 63u)) return DCDF_ERR_BAD_ARG;
        u192_add(acc, space_scaled(hi[i], lo[i], scale[i]));
    }
    *sum = space_round(acc);
    return DCDF_OK;
}
// the host masks of the cubes that have instants, one after the other in a pooled device buffer: cube q's at moff[q]
static int stage_cube_masks(const dcdf_cube* cubes, size_t nq, const uint8_t* mask, const uint64_t* mask_offset, const std::vector<uint64_t>& moff,
                            uint64_t mask_total, DevBuf& d_mask) {
    K2R_HIP(d_mask.alloc_pooled(mask_total));
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t bytes = (uint64_t)(c.bottom - c.top) * (c.right - c.left);
        if (c.end == c.start || bytes == 0) continue;
        K2R_HIP(hipMemcpy((uint8_t*)d_mask.p + moff[q], mask + mask_offset[q], bytes, hipMemcpyHostToDevice));
    }
    return DCDF_OK;
}
extern "C" int dcdf_raster_reduce_space_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint8_t* mask,
                                              const uint64_t* mask_offset, int mask_mem, double* out, int out_mem, const uint64_t* out_offset,
                                              uint64_t stats[3], float* kernel_ms) {
    if (!r || !cubes || !out || !out_offset || nq > 0x7fffffffu || ops == 0 || ops > (RA_ALL | ROP_MEAN) ||
        (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE) || (mask && !mask_offset) ||
        (mask && mask_mem != DCDF_MEM_HOST && mask_mem != DCDF_MEM_DEVICE))
        return DCDF_ERR_BAD_ARG;
    if (!r->all_wave || r->bad_fbits) return DCDF_ERR_UNSUPPORTED;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (kernel_ms) *kernel_ms = 0.f;
    if (nq == 0) return DCDF_OK;
    const uint32_t live = reduce_live(ops), n_out = popc32(ops);
    // where the series go: cube q's are n_out "instants" of one row of [instants] to WindowOut; where its mask bytes are
    std::vector<dcdf_cube> series(nq, dcdf_cube{});
    std::vector<uint64_t> moff(nq, 0);
    uint64_t mask_total = 0;
    const bool stage_mask = mask && mask_mem == DCDF_MEM_HOST;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
        if (c.end == c.start) continue;
        series[q] = dcdf_cube{0, n_out, 0, 1, 0, c.end - c.start};
        if (mask) {
            moff[q] = stage_mask ? mask_total : mask_offset[q];
            mask_total += (uint64_t)(c.bottom - c.top) * (c.right - c.left);
        }
    }
    WindowOut W(series.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    // the plan: batches of jobs whose records share the scratch, one after the other
    struct Slab {
        size_t item0, item1, fold0, fold1;
    };
    struct Batch {
        size_t unit0, unit1, const0, const1, slab0, slab1, job0, job1;
        uint32_t unit_nt, job_nt;  // the longest unit / job
    };
    std::vector<SpaceUnit> units;
    std::vector<SpaceFold> cfolds, wfolds;
    std::vector<WinItem> items;
    std::vector<Slab> slabs;
    std::vector<SpaceJob> jobs;
    std::vector<Batch> batches;
    const uint64_t rec_cap = space_record_cap(), slab_cap = reduce_slab_cells();
    uint64_t rec_used = 0, rec_max = 0, slab_used = 0, slab_max = 0, fold_nt = 1;
    uint64_t n_bulk = 0, n_walk = 0, n_const = 0;  // cells read
    Batch cur{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    Slab cur_slab{0, 0, 0, 0};
    auto flush_slab = [&] {
        cur_slab.item1 = items.size();
        cur_slab.fold1 = wfolds.size();
        if (cur_slab.fold1 > cur_slab.fold0) slabs.push_back(cur_slab);
        slab_max = std::max(slab_max, slab_used);
        cur_slab = Slab{items.size(), 0, wfolds.size(), 0};
        slab_used = 0;
    };
    auto flush_batch = [&] {
        flush_slab();
        // few units: a unit's instants in several workgroups (bulk_parts); each part writes its own instants' records
        const size_t nu = units.size() - cur.unit0;
        if (bulk_parts(nu, cur.unit_nt, bulk_wanted_units()) > 1) {
            std::vector<SpaceUnit> split;
            for (size_t i = cur.unit0; i < units.size(); i++) {
                const SpaceUnit& u = units[i];
                const uint32_t nt = u.t1 - u.t0, np = bulk_parts(nu, nt, bulk_wanted_units());
                for (uint32_t j = 0; j < np; j++) {
                    SpaceUnit v = u;
                    v.t0 = bulk_part(u.t0, nt, np, j);
                    v.t1 = bulk_part(u.t0, nt, np, j + 1);
                    v.rec = u.rec + (v.t0 - u.t0);
                    if (v.t1 > v.t0) split.push_back(v);
                }
            }
            units.resize(cur.unit0);
            units.insert(units.end(), split.begin(), split.end());
        }
        cur.unit1 = units.size();
        cur.const1 = cfolds.size();
        cur.slab1 = slabs.size();
        cur.job1 = jobs.size();
        if (cur.job1 > cur.job0) batches.push_back(cur);
        rec_max = std::max(rec_max, rec_used);
        rec_used = 0;
        cur = Batch{units.size(), 0, cfolds.size(), 0, slabs.size(), 0, jobs.size(), 0, 0, 0};
    };
    struct WalkPiece {  // a piece for the window walk: chunk, chunk-level cube, and its fold without slab offset and record
        uint32_t chunk;
        dcdf_cube k;
        SpaceFold f;
    };
    std::vector<SpaceUnit> tu;
    std::vector<SpaceFold> tc;
    std::vector<WalkPiece> tw;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end == c.start) continue;
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        for (uint32_t seg = c.start / r->cs; seg <= (c.end - 1) / r->cs; seg++) {
            const uint32_t s0 = seg * r->cs, ls = std::max(c.start, s0), le = std::min(c.end, s0 + r->cs);  // the cube's instants of this segment
            tu.clear();
            tc.clear();
            tw.clear();
            if (wr * wc)
                raster_pieces(r, dcdf_cube{ls, le, c.top, c.bottom, c.left, c.right}, [&](uint32_t cid, const dcdf_cube& l, uint32_t, uint32_t r0, uint32_t c0) {
                    const uint64_t m_off = moff[q] + (uint64_t)(r0 + l.top - c.top) * wc + (c0 + l.left - c.left);
                    const uint64_t cells = cube_cells(l);
                    const RasterLeaf f = r->tiled ? r->leaves[cid] : RasterLeaf{};
                    SpaceFold p{l.end - l.start, l.bottom - l.top, l.right - l.left, (uint32_t)wc, f.enc, f.fbits, 1u, 0u,
                                (uint64_t)cid * r->cs + l.start, 0, m_off};
                    if (f.elided) {
                        tc.push_back(p);
                        n_const += cells;
                        return;
                    }
                    const dcdf_chunk* h = r->chunks[cid];
                    const dcdf_cube k{l.start, l.end, f.row0 + l.top, f.row0 + l.bottom, f.col0 + l.left, f.col0 + l.right};  // chunk coordinates
                    if (!(h->top_g && h->narrow32)) {
                        p.enc = h->encoding;
                        p.fbits = h->fbits;
                        p.elided = 0;
                        tw.push_back(WalkPiece{cid, k, p});
                        n_walk += cells;
                        return;
                    }
                    for (uint32_t rr = k.top & ~(BULK_REGION - 1); rr < k.bottom; rr += BULK_REGION)
                        for (uint32_t rc = k.left & ~(BULK_REGION - 1); rc < k.right; rc += BULK_REGION) {
                            SpaceUnit u{};
                            u.chunk = cid;
                            u.t0 = k.start;
                            u.t1 = k.end;
                            u.rr = (uint16_t)rr;
                            u.rc = (uint16_t)rc;
                            u.top = (uint16_t)std::max(rr, k.top);
                            u.bottom = (uint16_t)std::min(rr + BULK_REGION, k.bottom);
                            u.left = (uint16_t)std::max(rc, k.left);
                            u.right = (uint16_t)std::min(rc + BULK_REGION, k.right);
                            u.m_sr = (uint32_t)wc;
                            u.m_off = m_off + (uint64_t)(u.top - k.top) * wc + (u.left - k.left);
                            tu.push_back(u);
                        }
                    n_bulk += cells;
                });
            // the segment's instants in jobs of at most rec_cap records (one job, but for a huge cube)
            const uint64_t n_slots = tu.size() + tc.size() + tw.size();
            const uint32_t nt = le - ls, step = n_slots ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, rec_cap / n_slots)) : nt;
            for (uint32_t a = 0; a < nt; a += step) {
                const uint32_t b = std::min(nt, a + step), jn = b - a;
                if (rec_used && rec_used + n_slots * jn > rec_cap) flush_batch();
                jobs.push_back(SpaceJob{rec_used, (uint32_t)n_slots, jn, W.base[q] + (ls + a - c.start), (uint64_t)(c.end - c.start)});
                uint64_t rec = rec_used;
                for (SpaceUnit u : tu) {
                    u.t0 += a;
                    u.t1 = u.t0 + jn;
                    u.rec = rec;
                    units.push_back(u);
                    rec += jn;
                }
                if (!tu.empty()) cur.unit_nt = std::max(cur.unit_nt, jn);
                for (SpaceFold p : tc) {
                    p.src += a;
                    p.nt = jn;
                    p.rec = rec;
                    cfolds.push_back(p);
                    rec += jn;
                }
                for (const WalkPiece& w : tw) {  // into slabs: whole pieces up to the cell bound, a piece beyond it cut in time
                    const uint64_t plane = (uint64_t)w.f.rows * w.f.cols;
                    const uint32_t cut = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(jn, slab_cap / plane));
                    if (cut < jn || slab_used + (uint64_t)jn * plane > slab_cap) flush_slab();
                    for (uint32_t x = 0; x < jn; x += cut) {
                        const uint32_t y = std::min(jn, x + cut);
                        dcdf_cube k = w.k;
                        k.start = w.k.start + a + x;
                        k.end = w.k.start + a + y;
                        SpaceFold p = w.f;
                        p.nt = y - x;
                        p.src = slab_used;
                        p.rec = rec + x;
                        window_items(w.chunk, k, slab_used, items, r->all_node);
                        wfolds.push_back(p);
                        fold_nt = std::max<uint64_t>(fold_nt, p.nt);
                        slab_used += (uint64_t)(y - x) * plane;
                        if (cut < jn) flush_slab();
                    }
                    rec += jn;
                }
                rec_used = rec;
                cur.job_nt = std::max(cur.job_nt, jn);
            }
            if (units.size() > 0x3fffffffull || items.size() > 0xfffffff0ull || cfolds.size() + wfolds.size() > 0xfffffff0ull ||
                jobs.size() > 0x7ffffff0ull)
                return DCDF_ERR_CAPACITY;
        }
    }
    flush_batch();
    if (stats) {
        stats[0] = n_bulk;
        stats[1] = n_walk;
        stats[2] = n_const;
    }
    if (W.total == 0) return DCDF_OK;
    DevBuf d_units, d_cfolds, d_wfolds, d_items, d_jobs, d_slab, d_recs, d_mask;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    double* const d_dst = (double*)W.dst();
    const uint8_t* p_mask = mask;
    if (stage_mask) {
        const int rcm = stage_cube_masks(cubes, nq, mask, mask_offset, moff, mask_total, d_mask);
        if (rcm != DCDF_OK) return rcm;
        p_mask = (const uint8_t*)d_mask.p;
    }
    K2R_HIP(d_recs.alloc_pooled(rec_max * sizeof(SpacePartial)));
    if (!units.empty()) K2R_HIP(upload(d_units, units));
    if (!cfolds.empty()) K2R_HIP(upload(d_cfolds, cfolds));
    if (!wfolds.empty()) K2R_HIP(upload(d_wfolds, wfolds));
    if (!items.empty()) K2R_HIP(upload(d_items, items));
    if (slab_max) K2R_HIP(d_slab.alloc_pooled(slab_max * sizeof(int64_t)));
    K2R_HIP(upload(d_jobs, jobs));
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    SpacePartial* const recs = d_recs.as<SpacePartial>();
    for (const Batch& b : batches) {
        if (b.const1 > b.const0) {
            hipLaunchKernelGGL(k_space_fold, dim3((uint32_t)std::min<size_t>(b.const1 - b.const0, 1u << 20), 1), dim3(256), 0, 0,
                               d_cfolds.as<SpaceFold>() + b.const0, (uint32_t)(b.const1 - b.const0), nullptr, r->d_vals.as<int64_t>(), p_mask, recs);
            K2R_HIP(hipGetLastError());
        }
        int rc = launch_bulk_space(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), d_units.as<SpaceUnit>() + b.unit0, (uint32_t)(b.unit1 - b.unit0),
                                   p_mask, recs, live);
        if (rc != DCDF_OK) return rc;
        for (size_t s = b.slab0; s < b.slab1; s++) {
            const Slab& sl = slabs[s];
            rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>() + sl.item0, (uint32_t)(sl.item1 - sl.item0), d_slab.p, DCDF_I64, nullptr,
                                         nullptr, r->all_node, r->all_narrow);
            if (rc != DCDF_OK) return rc;
            hipLaunchKernelGGL(k_space_fold, dim3((uint32_t)std::min<size_t>(sl.fold1 - sl.fold0, 1u << 20), (uint32_t)std::min<uint64_t>(fold_nt, 1024)),
                               dim3(256), 0, 0, d_wfolds.as<SpaceFold>() + sl.fold0, (uint32_t)(sl.fold1 - sl.fold0), d_slab.as<int64_t>(), nullptr,
                               p_mask, recs);
            K2R_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_space_finish, dim3((uint32_t)std::min<size_t>(b.job1 - b.job0, 1u << 20), std::min<uint32_t>(b.job_nt, 1024)), dim3(256), 0,
                           0, d_jobs.as<SpaceJob>() + b.job0, (uint32_t)(b.job1 - b.job0), recs, d_dst, ops);
        K2R_HIP(hipGetLastError());
    }
    K2R_HIP(hipEventRecord(ev.e1, 0));
    K2R_HIP(hipDeviceSynchronize());
    const int rcf = W.finish();
    if (rcf != DCDF_OK) return rcf;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
// ---- value histograms: per instant, how many selected cells of a cube fall into every bin of shared edges (k2r_hist.h) -------
// The pieces of every cube are classified as dcdf_raster_decode_batch classifies them.  Every piece -- a 64 x 64 unit of the bulk
// kernel, a piece of the window walk, an elided piece -- adds its counts to the cube's own [instants][bins] array with
// device-scope 64-bit atomic adds; the call zeroes exactly those arrays first.  Integer adds commute, so the work of all segments
// and cubes goes into one launch of each kind and the result depends on no order.
//
// A workgroup per (piece, instant) of the window walk's slab: the cells' stored integers widened by the leaf's own encoding and
// binned by the definition itself (hist_bin: the values here are wide, and the walk dominates), masked cells skipped, counts in
// an LDS histogram first.  An elided piece (blockIdx.y == 0 alone): its selected cells are counted once, then a thread per
// instant adds that count to the bin of the piece's value.
__global__ void __launch_bounds__(256)
k_hist_fold(const HistFold* __restrict__ ps, uint32_t n, const int64_t* __restrict__ slab, const int64_t* __restrict__ vals,
            const uint8_t* __restrict__ mask, const double* __restrict__ edges, uint32_t n_bins, uint64_t* out) {
    __shared__ uint32_t sh_cnt[HIST_MAX_BINS];
    __shared__ uint32_t sh_sel;
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const HistFold P = ps[p];
        const uint64_t cells = (uint64_t)P.rows * P.cols;
        if (P.elided) {
            if (blockIdx.y != 0) continue;
            __syncthreads();  // (the previous piece's readers are done)
            if (threadIdx.x == 0) sh_sel = mask ? 0u : (uint32_t)cells;
            __syncthreads();
            if (mask) {
                uint32_t c = 0;
                for (uint64_t e = threadIdx.x; e < cells; e += blockDim.x) c += mask[P.m_off + e / P.cols * P.m_sr + e % P.cols] != 0 ? 1u : 0u;
                if (c) atomicAdd(&sh_sel, c);
                __syncthreads();
            }
            const uint32_t selected = sh_sel;
            for (uint32_t t = threadIdx.x; t < P.nt && selected; t += blockDim.x) {
                const int32_t b = hist_bin(edges, n_bins, reduce_widen(P.enc, P.fbits, vals[P.src + t]));
                if (b >= 0) atomicAdd((unsigned long long*)out + (P.o_off + (uint64_t)t * n_bins + (uint32_t)b), (unsigned long long)selected);
            }
            continue;
        }
        for (uint32_t t = blockIdx.y; t < P.nt; t += gridDim.y) {
            __syncthreads();  // (the previous round's readers are done)
            for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x) sh_cnt[i] = 0u;
            __syncthreads();
            for (uint64_t e = threadIdx.x; e < cells; e += blockDim.x) {
                if (mask && mask[P.m_off + e / P.cols * P.m_sr + e % P.cols] == 0) continue;
                const int32_t b = hist_bin(edges, n_bins, reduce_widen(P.enc, P.fbits, slab[P.src + (uint64_t)t * cells + e]));
                if (b >= 0) atomicAdd(&sh_cnt[b], 1u);
            }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x) {
                const uint32_t c = sh_cnt[i];
                if (c) atomicAdd((unsigned long long*)out + (P.o_off + (uint64_t)t * n_bins + i), (unsigned long long)c);
            }
        }
    }
}
extern "C" int dcdf_histogram_bounds(int32_t encoding, uint32_t fractional_bits, const double* edges, uint32_t n_bins, int64_t* lo, int64_t* hi) {
    if (!lo || !hi || !hist_edges_ok(edges, n_bins) || !hist_leaf_ok(encoding, fractional_bits)) return DCDF_ERR_BAD_ARG;
    hist_intervals(encoding, fractional_bits, edges, n_bins, lo, hi);
    return DCDF_OK;
}
extern "C" int dcdf_raster_histogram_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const double* edges, uint32_t n_bins,
                                           const uint8_t* mask, const uint64_t* mask_offset, int mask_mem, uint64_t* out, int out_mem,
                                           const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    if (!r || !cubes || !out || !out_offset || nq > 0x7fffffffu || !hist_edges_ok(edges, n_bins) ||
        (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE) || (mask && !mask_offset) ||
        (mask && mask_mem != DCDF_MEM_HOST && mask_mem != DCDF_MEM_DEVICE))
        return DCDF_ERR_BAD_ARG;
    if (!r->all_wave || r->bad_fbits) return DCDF_ERR_UNSUPPORTED;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (kernel_ms) *kernel_ms = 0.f;
    if (nq == 0) return DCDF_OK;
    // where the counts go: cube q's are "instants" of one row of [bins] to WindowOut; where its mask bytes are
    std::vector<dcdf_cube> rows(nq, dcdf_cube{});
    std::vector<uint64_t> moff(nq, 0);
    uint64_t mask_total = 0;
    const bool stage_mask = mask && mask_mem == DCDF_MEM_HOST;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
        if (c.end == c.start) continue;
        rows[q] = dcdf_cube{0, c.end - c.start, 0, 1, 0, n_bins};
        if (mask) {
            moff[q] = stage_mask ? mask_total : mask_offset[q];
            mask_total += (uint64_t)(c.bottom - c.top) * (c.right - c.left);
        }
    }
    WindowOut W(rows.data(), nq, out, out_offset, sizeof(uint64_t), out_mem == DCDF_MEM_DEVICE);
    // the thresholds of every distinct (encoding, fractional bits) among the bulk kernel's leaves: translated once, here
    const uint32_t tab = (uint32_t)1 << hist_steps(n_bins);
    std::map<std::pair<int32_t, uint32_t>, uint32_t> leaf_thr;
    std::vector<int32_t> thr;
    struct Slab {
        size_t item0, item1, fold0, fold1;
    };
    std::vector<HistUnit> units;
    std::vector<HistFold> cfolds, wfolds;
    std::vector<WinItem> items;
    std::vector<Slab> slabs;
    const uint64_t slab_cap = reduce_slab_cells();
    uint64_t slab_used = 0, slab_max = 0, fold_nt = 1;
    uint64_t n_bulk = 0, n_walk = 0, n_const = 0;  // cells read
    uint32_t max_nt = 0;
    Slab cur_slab{0, 0, 0, 0};
    auto flush_slab = [&] {
        cur_slab.item1 = items.size();
        cur_slab.fold1 = wfolds.size();
        if (cur_slab.fold1 > cur_slab.fold0) slabs.push_back(cur_slab);
        slab_max = std::max(slab_max, slab_used);
        cur_slab = Slab{items.size(), 0, wfolds.size(), 0};
        slab_used = 0;
    };
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if ((uint64_t)(c.end - c.start) * wr * wc == 0) continue;
        raster_pieces(r, c, [&](uint32_t cid, const dcdf_cube& l, uint32_t t0, uint32_t r0, uint32_t c0) {
            const uint64_t m_off = moff[q] + (uint64_t)(r0 + l.top - c.top) * wc + (c0 + l.left - c.left);
            const uint64_t o_off = W.base[q] + (uint64_t)(t0 + l.start - c.start) * n_bins;
            const uint64_t cells = cube_cells(l);
            const RasterLeaf f = r->tiled ? r->leaves[cid] : RasterLeaf{};
            HistFold p{l.end - l.start, l.bottom - l.top, l.right - l.left, (uint32_t)wc, f.enc, f.fbits, 1u, 0u,
                       (uint64_t)cid * r->cs + l.start, o_off, m_off};
            if (f.elided) {
                cfolds.push_back(p);
                n_const += cells;
                return;
            }
            const dcdf_chunk* h = r->chunks[cid];
            const dcdf_cube k{l.start, l.end, f.row0 + l.top, f.row0 + l.bottom, f.col0 + l.left, f.col0 + l.right};  // chunk coordinates
            if (!(h->top_g && h->narrow32)) {  // into slabs: whole pieces up to the cell bound, a piece beyond it cut in time
                p.enc = h->encoding;
                p.fbits = h->fbits;
                p.elided = 0;
                const uint64_t plane = (uint64_t)p.rows * p.cols;
                const uint32_t nt = p.nt, cut = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, slab_cap / plane));
                if (cut < nt || slab_used + (uint64_t)nt * plane > slab_cap) flush_slab();
                for (uint32_t x = 0; x < nt; x += cut) {
                    const uint32_t y = std::min(nt, x + cut);
                    dcdf_cube kk = k;
                    kk.start = k.start + x;
                    kk.end = k.start + y;
                    HistFold w = p;
                    w.nt = y - x;
                    w.src = slab_used;
                    w.o_off = o_off + (uint64_t)x * n_bins;
                    window_items(cid, kk, slab_used, items, r->all_node);
                    wfolds.push_back(w);
                    fold_nt = std::max<uint64_t>(fold_nt, w.nt);
                    slab_used += (uint64_t)(y - x) * plane;
                    if (cut < nt) flush_slab();
                }
                n_walk += cells;
                return;
            }
            const auto key = std::make_pair((int32_t)h->encoding, (uint32_t)h->fbits);
            auto it = leaf_thr.find(key);
            if (it == leaf_thr.end()) {
                it = leaf_thr.emplace(key, (uint32_t)thr.size()).first;
                thr.resize(thr.size() + tab);
                hist_thresholds32(key.first, key.second, edges, n_bins, thr.data() + it->second, tab);
            }
            for (uint32_t rr = k.top & ~(BULK_REGION - 1); rr < k.bottom; rr += BULK_REGION)
                for (uint32_t rc = k.left & ~(BULK_REGION - 1); rc < k.right; rc += BULK_REGION) {
                    HistUnit u{};
                    u.chunk = cid;
                    u.t0 = k.start;
                    u.t1 = k.end;
                    u.rr = (uint16_t)rr;
                    u.rc = (uint16_t)rc;
                    u.top = (uint16_t)std::max(rr, k.top);
                    u.bottom = (uint16_t)std::min(rr + BULK_REGION, k.bottom);
                    u.left = (uint16_t)std::max(rc, k.left);
                    u.right = (uint16_t)std::min(rc + BULK_REGION, k.right);
                    u.m_sr = (uint32_t)wc;
                    u.thr = it->second;
                    u.rev = hist_reversed(key.first, key.second) ? 1u : 0u;
                    u.o_off = o_off;
                    u.m_off = m_off + (uint64_t)(u.top - k.top) * wc + (u.left - k.left);
                    units.push_back(u);
                }
            max_nt = std::max(max_nt, k.end - k.start);
            n_bulk += cells;
        });
        if (units.size() > 0x3fffffffull || items.size() > 0xfffffff0ull || cfolds.size() + wfolds.size() > 0xfffffff0ull ||
            thr.size() > 0x7fffffffull)
            return DCDF_ERR_CAPACITY;
    }
    flush_slab();
    if (stats) {
        stats[0] = n_bulk;
        stats[1] = n_walk;
        stats[2] = n_const;
    }
    if (W.total == 0) return DCDF_OK;
    // few units: a unit's instants in several workgroups (bulk_parts); each part adds to its own instants' rows
    if (bulk_parts(units.size(), max_nt, bulk_wanted_units()) > 1) {
        std::vector<HistUnit> split;
        split.reserve(units.size() * 2);
        for (const HistUnit& u : units) {
            const uint32_t nt = u.t1 - u.t0, np = bulk_parts(units.size(), nt, bulk_wanted_units());
            for (uint32_t j = 0; j < np; j++) {
                HistUnit v = u;
                v.t0 = bulk_part(u.t0, nt, np, j);
                v.t1 = bulk_part(u.t0, nt, np, j + 1);
                v.o_off = u.o_off + (uint64_t)(v.t0 - u.t0) * n_bins;
                if (v.t1 > v.t0) split.push_back(v);
            }
        }
        units.swap(split);
    }
    DevBuf d_units, d_cfolds, d_wfolds, d_items, d_slab, d_mask, d_thr, d_edges;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    uint64_t* const d_dst = (uint64_t*)W.dst();
    const uint8_t* p_mask = mask;
    if (stage_mask) {
        const int rcm = stage_cube_masks(cubes, nq, mask, mask_offset, moff, mask_total, d_mask);
        if (rcm != DCDF_OK) return rcm;
        p_mask = (const uint8_t*)d_mask.p;
    }
    if (!units.empty()) {
        K2R_HIP(upload(d_units, units));
        K2R_HIP(upload(d_thr, thr));
    }
    if (!cfolds.empty()) K2R_HIP(upload(d_cfolds, cfolds));
    if (!wfolds.empty()) K2R_HIP(upload(d_wfolds, wfolds));
    if (!items.empty()) K2R_HIP(upload(d_items, items));
    if (slab_max) K2R_HIP(d_slab.alloc_pooled(slab_max * sizeof(int64_t)));
    if (!cfolds.empty() || !wfolds.empty()) K2R_HIP(upload(d_edges, std::vector<double>(edges, edges + n_bins + 1)));
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    // the accumulators: exactly the cubes' arrays, nothing between them
    if (!W.to_dev) {
        K2R_HIP(hipMemsetAsync(d_dst, 0, W.total * W.es, 0));
    } else {
        for (size_t q = 0; q < nq; q++) {
            const uint64_t n = cube_cells(rows[q]);
            if (n) K2R_HIP(hipMemsetAsync(d_dst + W.base[q], 0, n * sizeof(uint64_t), 0));
        }
    }
    if (!cfolds.empty()) {
        hipLaunchKernelGGL(k_hist_fold, dim3((uint32_t)std::min<size_t>(cfolds.size(), 1u << 20), 1), dim3(256), 0, 0, d_cfolds.as<HistFold>(),
                           (uint32_t)cfolds.size(), nullptr, r->d_vals.as<int64_t>(), p_mask, d_edges.as<double>(), n_bins, d_dst);
        K2R_HIP(hipGetLastError());
    }
    int rc = launch_bulk_hist(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), d_units.as<HistUnit>(), (uint32_t)units.size(), p_mask,
                              d_thr.as<int32_t>(), n_bins, d_dst);
    if (rc != DCDF_OK) return rc;
    for (const Slab& sl : slabs) {
        rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>() + sl.item0, (uint32_t)(sl.item1 - sl.item0), d_slab.p, DCDF_I64, nullptr,
                                     nullptr, r->all_node, r->all_narrow);
        if (rc != DCDF_OK) return rc;
        hipLaunchKernelGGL(k_hist_fold, dim3((uint32_t)std::min<size_t>(sl.fold1 - sl.fold0, 1u << 20), (uint32_t)std::min<uint64_t>(fold_nt, 1024)),
                           dim3(256), 0, 0, d_wfolds.as<HistFold>() + sl.fold0, (uint32_t)(sl.fold1 - sl.fold0), d_slab.as<int64_t>(), nullptr,
                           p_mask, d_edges.as<double>(), n_bins, d_dst);
        K2R_HIP(hipGetLastError());
    }
    K2R_HIP(hipEventRecord(ev.e1, 0));
    K2R_HIP(hipDeviceSynchronize());
    const int rcf = W.finish();
    if (rcf != DCDF_OK) return rcf;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
// ---- search of dataset-level cubes with everything but a count per cube on the device ---------------------------------
// One thread per cube writes what search_impl builds on the host: a WinQuery per chunk-level piece (with the chunk's origin
// for the emit kernel), a SearchItem per (piece, instant), a WinItem + SearchExtra per <= 64 x 64 part of it.
// VALUE: the cube's bounds are real values (vlower / vupper); each piece translates them with its chunk's encoding (enc) and
// fractional bits (value_bounds, the definition the host uses), the per-item flag is the hole instead of the reference quirk, and
// a piece whose range is empty (or, narrow: misses the int32 range its walk covers) gets [INT64_MAX, INT64_MIN]: nothing matches
// and the walk's side-16 table prunes every square of it.
template <bool VALUE>
__device__ __forceinline__ void raster_search_expand(const dcdf_cube* __restrict__ cubes, const int64_t* __restrict__ lower,
                                                     const int64_t* __restrict__ upper, const double* __restrict__ vlower,
                                                     const double* __restrict__ vupper, const uint32_t* __restrict__ sb,
                                                     const uint32_t* __restrict__ ib, const uint32_t* __restrict__ wb, uint32_t nq, RasterGeom g,
                                                     const uint8_t* __restrict__ quirk, const ChunkRef* __restrict__ refs,
                                                     const uint8_t* __restrict__ enc, bool narrow, WinQuery* __restrict__ qs,
                                                     SearchItem* __restrict__ items, WinItem* __restrict__ witems, SearchExtra* __restrict__ sx) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    dcdf_cube c = cubes[q];
    if (c.start > c.end) { const uint32_t x = c.start; c.start = c.end; c.end = x; }
    if (c.top > c.bottom) { const uint32_t x = c.top; c.top = c.bottom; c.bottom = x; }
    if (c.left > c.right) { const uint32_t x = c.left; c.left = c.right; c.right = x; }
    if ((uint64_t)(c.end - c.start) * (c.bottom - c.top) * (c.right - c.left) == 0) return;
    int64_t lo = 0, hi = 0;
    if (!VALUE) {
        lo = min(lower[q], upper[q]);  // helpers.rs:7-16 via chunk.rs:214
        hi = max(lower[q], upper[q]);
    }
    uint32_t s = sb[q], it = ib[q], w = wb[q];
    for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++)
        for (uint32_t ti = c.top / g.tile; ti <= (c.bottom - 1) / g.tile; ti++)
            for (uint32_t tj = c.left / g.tile; tj <= (c.right - 1) / g.tile; tj++) {
                const uint32_t t0 = seg * g.cs, r0 = ti * g.tile, c0 = tj * g.tile;
                const uint32_t ls = max(c.start, t0) - t0, le = min(c.end, t0 + g.cs) - t0, lt = max(c.top, r0) - r0, lb = min(c.bottom, r0 + g.tile) - r0,
                               ll = max(c.left, c0) - c0, lr = min(c.right, c0 + g.tile) - c0;
                const uint32_t cid = (seg * g.nti + ti) * g.ntj + tj;
                bool hole = false;
                if (VALUE) {
                    ValueRange vr;
                    (void)value_bounds((int32_t)enc[cid], refs[cid].fbits, vlower[q], vupper[q], &vr);  // (the host checked the arguments)
                    if (!vr.empty && narrow) {
                        vr.lo = max(vr.lo, (int64_t)INT32_MIN);
                        vr.hi = min(vr.hi, (int64_t)INT32_MAX);
                        vr.empty = vr.lo > vr.hi;
                    }
                    lo = vr.empty ? INT64_MAX : vr.lo;
                    hi = vr.empty ? INT64_MIN : vr.hi;
                    hole = !vr.empty && vr.hole;
                }
                WinQuery Q;
                Q.chunk = cid;
                Q.start = ls; Q.end = le; Q.top = lt; Q.bottom = lb; Q.left = ll; Q.right = lr;
                Q._pad = t0;  // the chunk's origin inside the raster, added to every triple by k_search_emit
                Q.lower = lo;
                Q.upper = hi;
                Q.out_off = (uint64_t)r0 | (uint64_t)c0 << 32;
                qs[s] = Q;
                const uint32_t ncb = (lr - ll + 63u) >> 6;
                for (uint32_t t = ls; t < le; t++) {
                    items[it++] = SearchItem{s, t, 0, w, ncb};
                    const uint32_t qk = VALUE ? (hole ? 1u : 0u) : quirk[(size_t)cid * g.cs + t];
                    for (uint32_t rr = lt; rr < lb; rr += 64)
                        for (uint32_t cc = ll; cc < lr; cc += 64) {
                            WinItem wi;
                            wi.chunk = cid;
                            wi.inst = t;
                            wi.top = (uint16_t)rr;
                            wi.bottom = (uint16_t)min(rr + 64, lb);
                            wi.left = (uint16_t)cc;
                            wi.right = (uint16_t)min(cc + 64, lr);
                            wi.out_sr = 0;
                            wi.out_off = 0;
                            witems[w] = wi;
                            sx[w] = SearchExtra{lo, hi, qk, 0u};
                            w++;
                        }
                }
                s++;
            }
}
__global__ void __launch_bounds__(256)
k_raster_search_expand(const dcdf_cube* __restrict__ cubes, const int64_t* __restrict__ lower, const int64_t* __restrict__ upper,
                       const uint32_t* __restrict__ sb, const uint32_t* __restrict__ ib, const uint32_t* __restrict__ wb, uint32_t nq, RasterGeom g,
                       const uint8_t* __restrict__ quirk, WinQuery* __restrict__ qs, SearchItem* __restrict__ items, WinItem* __restrict__ witems,
                       SearchExtra* __restrict__ sx) {
    raster_search_expand<false>(cubes, lower, upper, nullptr, nullptr, sb, ib, wb, nq, g, quirk, nullptr, nullptr, false, qs, items, witems, sx);
}
__global__ void __launch_bounds__(256)
k_raster_search_values_expand(const dcdf_cube* __restrict__ cubes, const double* __restrict__ lower, const double* __restrict__ upper,
                              const uint32_t* __restrict__ sb, const uint32_t* __restrict__ ib, const uint32_t* __restrict__ wb, uint32_t nq,
                              RasterGeom g, const ChunkRef* __restrict__ refs, const uint8_t* __restrict__ enc, uint32_t narrow,
                              WinQuery* __restrict__ qs, SearchItem* __restrict__ items, WinItem* __restrict__ witems, SearchExtra* __restrict__ sx) {
    raster_search_expand<true>(cubes, nullptr, nullptr, lower, upper, sb, ib, wb, nq, g, nullptr, refs, enc, narrow != 0, qs, items, witems, sx);
}
// exclusive prefix sum of n uint32 counts into uint64 offsets: block sums, their scan by one block, the offsets
constexpr uint32_t kScanPer = 2048;  // elements per 256-thread block
__global__ void __launch_bounds__(256) k_scan_sums(const uint32_t* __restrict__ v, uint32_t n, uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[256];
    const uint32_t b0 = blockIdx.x * kScanPer;
    uint64_t a = 0;
    for (uint32_t i = threadIdx.x; i < kScanPer && b0 + i < n; i += 256) a += v[b0 + i];
    part[threadIdx.x] = a;
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}
__global__ void __launch_bounds__(256) k_scan_top(uint64_t* __restrict__ sums, uint32_t nb, uint64_t* __restrict__ total) {
    // (one block; nb is small: n / 2048) sums[b] <- sum of the blocks before b
    __shared__ uint64_t part[256];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
        const uint32_t i = b0 + threadIdx.x;
        const uint64_t x = i < nb ? sums[i] : 0;
        part[threadIdx.x] = x;
        __syncthreads();
        for (uint32_t st = 1; st < 256; st <<= 1) {  // inclusive scan (Hillis-Steele)
            const uint64_t y = threadIdx.x >= st ? part[threadIdx.x - st] : 0;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (i < nb) sums[i] = carry + part[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 255) carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(256) k_scan_apply(const uint32_t* __restrict__ v, uint32_t n, const uint64_t* __restrict__ sums,
                                                    uint64_t* __restrict__ offs) {
    // thread t of the block owns 8 consecutive elements: its prefix inside the block by a scan of the threads' sums
    __shared__ uint64_t part[256];
    const uint32_t b0 = blockIdx.x * kScanPer + threadIdx.x * 8;
    uint32_t x[8];
    uint64_t a = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        x[j] = b0 + j < n ? v[b0 + j] : 0u;
        a += x[j];
    }
    part[threadIdx.x] = a;
    __syncthreads();
    for (uint32_t st = 1; st < 256; st <<= 1) {
        const uint64_t y = threadIdx.x >= st ? part[threadIdx.x - st] : 0;
        __syncthreads();
        part[threadIdx.x] += y;
        __syncthreads();
    }
    uint64_t run = sums[blockIdx.x] + part[threadIdx.x] - a;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (b0 + j < n) offs[b0 + j] = run;
        run += x[j];
    }
}
// per cube: where its triples begin and how many there are (its items are consecutive)
__global__ void __launch_bounds__(256) k_raster_query_counts(const uint32_t* __restrict__ ib, uint32_t nq, uint32_t ni, const uint64_t* __restrict__ offs,
                                                             const uint64_t* __restrict__ total, uint64_t* __restrict__ counts,
                                                             uint64_t* __restrict__ offsets) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t a = ib[q], b = ib[q + 1];
    const uint64_t oa = a < ni ? offs[a] : *total, ob = b < ni ? offs[b] : *total;
    offsets[q] = oa;
    counts[q] = ob - oa;
}

// ---- tiled rasters: search --------------------------------------------------------------------------------------------------
// A piece on an elided leaf is one further item kind of the walk -> count -> scan -> emit pipeline: a SearchItem per instant
// with w0 = SI_CONST and ncb = 1 when the leaf's value at that instant is in range (decided here, once), no wave items; it
// counts its whole area and emits it in (row, col) order.  A chunk piece whose leaf's holding node fails has_cells over the
// piece's instants (Superchunk::search, superchunk.rs:480-493), or, for a value search, whose exact (min, max) miss the range,
// keeps its items with the bounds [INT64_MAX, INT64_MIN]: the walk finds nothing there and the host's item counts stay valid.
constexpr uint32_t SI_CONST = 0xfffffffeu;
template <bool VALUE>
__global__ void __launch_bounds__(256)
k_raster_tiled_search_expand(const dcdf_cube* __restrict__ cubes, const int64_t* __restrict__ lower, const int64_t* __restrict__ upper,
                             const double* __restrict__ vlower, const double* __restrict__ vupper, const uint32_t* __restrict__ sb,
                             const uint32_t* __restrict__ ib, const uint32_t* __restrict__ wb, uint32_t nq, RasterGeom g,
                             const uint8_t* __restrict__ quirk, const ChunkRef* __restrict__ refs, const uint8_t* __restrict__ enc,
                             const RasterLeaf* __restrict__ leaves, const int64_t* __restrict__ vals, const int64_t* __restrict__ mm,
                             uint32_t narrow, WinQuery* __restrict__ qs, SearchItem* __restrict__ items, WinItem* __restrict__ witems,
                             SearchExtra* __restrict__ sx) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    dcdf_cube c = cubes[q];
    if (c.start > c.end) { const uint32_t x = c.start; c.start = c.end; c.end = x; }
    if (c.top > c.bottom) { const uint32_t x = c.top; c.top = c.bottom; c.bottom = x; }
    if (c.left > c.right) { const uint32_t x = c.left; c.left = c.right; c.right = x; }
    if ((uint64_t)(c.end - c.start) * (c.bottom - c.top) * (c.right - c.left) == 0) return;
    int64_t qlo = 0, qhi = 0;
    if (!VALUE) {
        qlo = min(lower[q], upper[q]);  // helpers.rs:7-16 via chunk.rs:214
        qhi = max(lower[q], upper[q]);
    }
    uint32_t s = sb[q], it = ib[q], w = wb[q];
    for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++)
        for (uint32_t ti = c.top / g.tile; ti <= (c.bottom - 1) / g.tile; ti++)
            for (uint32_t tj = c.left / g.tile; tj <= (c.right - 1) / g.tile; tj++) {
                const uint32_t t0 = seg * g.cs, r0 = ti * g.tile, c0 = tj * g.tile;
                const uint32_t ls = max(c.start, t0) - t0, le = min(c.end, t0 + g.cs) - t0, lt = max(c.top, r0) - r0, lb = min(c.bottom, r0 + g.tile) - r0,
                               ll = max(c.left, c0) - c0, lr = min(c.right, c0 + g.tile) - c0;
                const uint32_t cid = (seg * g.nti + ti) * g.ntj + tj;
                const RasterLeaf f = leaves[cid];
                const bool fenc = f.enc == ENC_F32 || f.enc == ENC_F64;
                // the leaf's bounds in the encoding and bits of its node (elided values, minmax)
                int64_t nlo = qlo, nhi = qhi;
                bool nhole = false;
                if (VALUE) {
                    ValueRange vr;
                    (void)value_bounds(f.enc, f.fbits, vlower[q], vupper[q], &vr);  // (checked at create)
                    nlo = vr.empty ? INT64_MAX : vr.lo;
                    nhi = vr.empty ? INT64_MIN : vr.hi;
                    nhole = !vr.empty && vr.hole;
                }
                WinQuery Q;
                Q.chunk = cid;
                Q.start = ls; Q.end = le;
                Q._pad = t0;
                if (f.elided) {
                    Q.top = lt; Q.bottom = lb; Q.left = ll; Q.right = lr;
                    Q.lower = nlo;
                    Q.upper = nhi;
                    Q.out_off = (uint64_t)r0 | (uint64_t)c0 << 32;
                    qs[s] = Q;
                    for (uint32_t t = ls; t < le; t++) {  // superchunk.rs:541-558: every cell of an instant in range
                        const int64_t v = vals[(size_t)cid * g.cs + t];
                        const bool hit = nlo <= v && v <= nhi && !(nhole && v == 0);
                        items[it++] = SearchItem{s, t, 0, SI_CONST, hit ? 1u : 0u};
                    }
                    s++;
                    continue;
                }
                int64_t lo = qlo, hi = qhi;
                bool hole = false;
                if (VALUE) {
                    ValueRange vr;
                    (void)value_bounds((int32_t)enc[cid], refs[cid].fbits, vlower[q], vupper[q], &vr);  // (the host checked the arguments)
                    if (!vr.empty && narrow) {
                        vr.lo = max(vr.lo, (int64_t)INT32_MIN);
                        vr.hi = min(vr.hi, (int64_t)INT32_MAX);
                        vr.empty = vr.lo > vr.hi;
                    }
                    lo = vr.empty ? INT64_MAX : vr.lo;
                    hi = vr.empty ? INT64_MIN : vr.hi;
                    hole = !vr.empty && vr.hole;
                }
                // has_cells (integer search of integer rasters) / exact-min-max pruning (value search; never at an instant whose float
                // min or max is 0, the NaN code)
                if (f.has_mm && (VALUE ? (bool)f.exact : !fenc)) {
                    bool live = false;
                    for (uint32_t t = ls; t < le && !live; t++) {
                        const int64_t mn = mm[((size_t)cid * g.cs + t) * 2], mx = mm[((size_t)cid * g.cs + t) * 2 + 1];
                        live = nhi >= mn && nlo <= mx;
                        if (VALUE && fenc) live = live || mn == 0 || mx == 0;
                    }
                    if (!live) {
                        lo = INT64_MAX;
                        hi = INT64_MIN;
                    }
                }
                const uint32_t ct = f.row0 + lt, cb = f.row0 + lb, cl = f.col0 + ll, cr = f.col0 + lr;  // chunk coordinates
                Q.top = ct; Q.bottom = cb; Q.left = cl; Q.right = cr;
                Q.lower = lo;
                Q.upper = hi;
                Q.out_off = (uint64_t)(r0 - f.row0) | (uint64_t)(c0 - f.col0) << 32;  // the chunk's origin inside the raster
                qs[s] = Q;
                const uint32_t ncb = (cr - cl + 63u) >> 6;
                for (uint32_t t = ls; t < le; t++) {
                    items[it++] = SearchItem{s, t, 0, w, ncb};
                    const uint32_t qk = VALUE ? (hole ? 1u : 0u) : quirk[(size_t)cid * g.cs + t];
                    for (uint32_t rr = ct; rr < cb; rr += 64)
                        for (uint32_t cc = cl; cc < cr; cc += 64) {
                            WinItem wi;
                            wi.chunk = cid;
                            wi.inst = t;
                            wi.top = (uint16_t)rr;
                            wi.bottom = (uint16_t)min(rr + 64, cb);
                            wi.left = (uint16_t)cc;
                            wi.right = (uint16_t)min(cc + 64, cr);
                            wi.out_sr = 0;
                            wi.out_off = 0;
                            witems[w] = wi;
                            sx[w] = SearchExtra{lo, hi, qk, 0u};
                            w++;
                        }
                }
                s++;
            }
}
__global__ void __launch_bounds__(64)
k_raster_tiled_search_count(const uint32_t* __restrict__ wbits, const SearchItem* __restrict__ items, const WinQuery* __restrict__ qs, uint32_t n,
                            uint32_t* __restrict__ counts) {
    const uint32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n) return;
    const SearchItem I = items[it];
    const WinQuery Q = qs[I.query];
    if (I.w0 == SI_CONST) counts[it] = I.ncb ? (Q.bottom - Q.top) * (Q.right - Q.left) : 0u;
    else counts[it] = search_count_wave_item(wbits, I, Q);
}
__global__ void __launch_bounds__(64)
k_raster_tiled_search_emit(const WinQuery* __restrict__ qs, const SearchItem* __restrict__ items, uint32_t n_items,
                           const uint32_t* __restrict__ wbits, const uint64_t* __restrict__ offs, uint32_t* __restrict__ out) {
    const uint32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_items) return;
    const SearchItem I = items[it];
    const WinQuery Q = qs[I.query];
    uint32_t* o = out + 3 * offs[it];
    if (I.w0 != SI_CONST) {
        search_emit_wave_item(I, Q, wbits, o);
        return;
    }
    if (!I.ncb) return;
    const uint32_t ot = Q._pad + I.instant, orow = (uint32_t)Q.out_off, ocol = (uint32_t)(Q.out_off >> 32);
    for (uint32_t r = Q.top; r < Q.bottom; r++)
        for (uint32_t c = Q.left; c < Q.right; c++) {
            o[0] = ot;
            o[1] = orow + r;
            o[2] = ocol + c;
            o += 3;
        }
}

// vlower / vupper (value search, lower / upper unused): real-valued bounds, translated per piece on the device
static int raster_search_device(const dcdf_raster* r, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper, size_t nq, uint32_t* out,
                                size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets, float* kernel_ms,
                                const double* vlower = nullptr, const double* vupper = nullptr) {
    const bool value = vlower != nullptr;
    std::vector<uint32_t> sb(nq + 1), ib(nq + 1), wb(nq + 1);
    uint64_t ns = 0, ni = 0, nw = 0;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
        sb[q] = (uint32_t)ns; ib[q] = (uint32_t)ni; wb[q] = (uint32_t)nw;
        if (cube_cells(c) == 0) continue;
        const uint64_t tiles = (uint64_t)((c.bottom - 1) / r->tile - c.top / r->tile + 1) * ((c.right - 1) / r->tile - c.left / r->tile + 1);
        ns += ((c.end - 1) / r->cs - c.start / r->cs + 1) * tiles;
        ni += (uint64_t)(c.end - c.start) * tiles;
        if (r->tiled) {  // (elided pieces make items but no wave items)
            uint64_t n_const = 0;
            tiled_item_count(r, c, 64, &nw, &n_const);
        } else {
            nw += raster_item_count(r, c, 64);
        }
        if (nw + 4096 > 0xffffff00ull) return DCDF_ERR_CAPACITY;
    }
    sb[nq] = (uint32_t)ns; ib[nq] = (uint32_t)ni; wb[nq] = (uint32_t)nw;
    for (size_t q = 0; q < nq; q++) counts[q] = offsets[q] = 0;
    if (ni == 0) {
        if (kernel_ms) *kernel_ms = 0.f;
        return DCDF_OK;
    }
    DevBuf d_cubes, d_lo, d_hi, d_sb, d_ib, d_wb, d_qs, d_items, d_witems, d_sx, d_wbits, d_counts, d_sums, d_total, d_offs, d_qc, d_qo, d_out;
    K2R_HIP(upload(d_cubes, cubes, nq * sizeof(dcdf_cube)));
    K2R_HIP(upload(d_lo, value ? (const void*)vlower : (const void*)lower, nq * 8));  // (8 bytes either way)
    K2R_HIP(upload(d_hi, value ? (const void*)vupper : (const void*)upper, nq * 8));
    K2R_HIP(upload(d_sb, sb));
    K2R_HIP(upload(d_ib, ib));
    K2R_HIP(upload(d_wb, wb));
    K2R_HIP(d_qs.alloc_pooled(ns * sizeof(WinQuery)));
    K2R_HIP(d_items.alloc_pooled(ni * sizeof(SearchItem)));
    K2R_HIP(d_witems.alloc_pooled(nw * sizeof(WinItem)));
    K2R_HIP(d_sx.alloc_pooled(nw * sizeof(SearchExtra)));
    K2R_HIP(d_wbits.alloc_pooled(nw * 512));  // (every word is written by the walk: nothing to clear)
    K2R_HIP(d_counts.alloc(ni * 4));
    K2R_HIP(d_offs.alloc(ni * 8));
    const uint32_t nb = (uint32_t)((ni + kScanPer - 1) / kScanPer);
    K2R_HIP(d_sums.alloc((size_t)nb * 8));
    K2R_HIP(d_total.alloc(8));
    K2R_HIP(d_qc.alloc(nq * 8));
    K2R_HIP(d_qo.alloc(nq * 8));
    EventPair ev;
    K2R_HIP(ev.create());
    const RasterGeom g{r->T, r->R, r->C, r->tile, r->cs, r->nti, r->ntj, 64u};
    const uint32_t nw32 = (uint32_t)nw, ni32 = (uint32_t)ni, nq32 = (uint32_t)nq;
    if (r->tiled && value)
        hipLaunchKernelGGL(k_raster_tiled_search_expand<true>, dim3((nq32 + 255) / 256), dim3(256), 0, 0, d_cubes.as<dcdf_cube>(), nullptr, nullptr,
                           d_lo.as<double>(), d_hi.as<double>(), d_sb.as<uint32_t>(), d_ib.as<uint32_t>(), d_wb.as<uint32_t>(), nq32, g,
                           r->d_quirk.as<uint8_t>(), r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), r->d_leaf.as<RasterLeaf>(),
                           r->d_vals.as<int64_t>(), r->d_mm.as<int64_t>(), r->all_narrow ? 1u : 0u, d_qs.as<WinQuery>(), d_items.as<SearchItem>(),
                           d_witems.as<WinItem>(), d_sx.as<SearchExtra>());
    else if (r->tiled)
        hipLaunchKernelGGL(k_raster_tiled_search_expand<false>, dim3((nq32 + 255) / 256), dim3(256), 0, 0, d_cubes.as<dcdf_cube>(), d_lo.as<int64_t>(),
                           d_hi.as<int64_t>(), nullptr, nullptr, d_sb.as<uint32_t>(), d_ib.as<uint32_t>(), d_wb.as<uint32_t>(), nq32, g,
                           r->d_quirk.as<uint8_t>(), r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), r->d_leaf.as<RasterLeaf>(),
                           r->d_vals.as<int64_t>(), r->d_mm.as<int64_t>(), r->all_narrow ? 1u : 0u, d_qs.as<WinQuery>(), d_items.as<SearchItem>(),
                           d_witems.as<WinItem>(), d_sx.as<SearchExtra>());
    else if (value)
        hipLaunchKernelGGL(k_raster_search_values_expand, dim3((nq32 + 255) / 256), dim3(256), 0, 0, d_cubes.as<dcdf_cube>(), d_lo.as<double>(),
                           d_hi.as<double>(), d_sb.as<uint32_t>(), d_ib.as<uint32_t>(), d_wb.as<uint32_t>(), nq32, g, r->d_refs.as<ChunkRef>(),
                           r->d_enc.as<uint8_t>(), r->all_narrow ? 1u : 0u, d_qs.as<WinQuery>(), d_items.as<SearchItem>(), d_witems.as<WinItem>(),
                           d_sx.as<SearchExtra>());
    else
        hipLaunchKernelGGL(k_raster_search_expand, dim3((nq32 + 255) / 256), dim3(256), 0, 0, d_cubes.as<dcdf_cube>(), d_lo.as<int64_t>(), d_hi.as<int64_t>(),
                           d_sb.as<uint32_t>(), d_ib.as<uint32_t>(), d_wb.as<uint32_t>(), nq32, g, r->d_quirk.as<uint8_t>(), d_qs.as<WinQuery>(),
                           d_items.as<SearchItem>(), d_witems.as<WinItem>(), d_sx.as<SearchExtra>());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    int rc = DCDF_OK;
    if (nw32)  // (0: a tiled raster whose pieces are all elided, nothing to walk)
        rc = launch_search_walk(r->d_refs.as<ChunkRef>(), d_witems.as<WinItem>(), nw32, d_wbits.p, d_sx.as<SearchExtra>(), r->all_narrow, value);
    if (rc != DCDF_OK) return rc;
    if (r->tiled)
        hipLaunchKernelGGL(k_raster_tiled_search_count, dim3((ni32 + 63) / 64), dim3(64), 0, 0, d_wbits.as<uint32_t>(), d_items.as<SearchItem>(),
                           d_qs.as<WinQuery>(), ni32, d_counts.as<uint32_t>());
    else
        rc = launch_search_count(d_wbits.as<uint32_t>(), d_items.as<SearchItem>(), d_qs.as<WinQuery>(), ni32, d_counts.as<uint32_t>());
    if (rc != DCDF_OK) return rc;
    hipLaunchKernelGGL(k_scan_sums, dim3(nb), dim3(256), 0, 0, d_counts.as<uint32_t>(), ni32, d_sums.as<uint64_t>());
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, 0, d_sums.as<uint64_t>(), nb, d_total.as<uint64_t>());
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, 0, d_counts.as<uint32_t>(), ni32, d_sums.as<uint64_t>(), d_offs.as<uint64_t>());
    hipLaunchKernelGGL(k_raster_query_counts, dim3((nq32 + 255) / 256), dim3(256), 0, 0, d_ib.as<uint32_t>(), nq32, ni32, d_offs.as<uint64_t>(),
                       d_total.as<uint64_t>(), d_qc.as<uint64_t>(), d_qo.as<uint64_t>());
    K2R_HIP(hipGetLastError());
    uint64_t total = 0;
    K2R_HIP(hipMemcpy(&total, d_total.p, 8, hipMemcpyDeviceToHost));
    K2R_HIP(hipMemcpy(counts, d_qc.p, nq * 8, hipMemcpyDeviceToHost));
    K2R_HIP(hipMemcpy(offsets, d_qo.p, nq * 8, hipMemcpyDeviceToHost));
    if (total > cap) return DCDF_ERR_CAPACITY;
    const bool to_dev = out_mem == DCDF_MEM_DEVICE;
    if (total > 0) {
        if (!to_dev) K2R_HIP(d_out.alloc_pooled(total * 12));
        if (r->tiled)
            hipLaunchKernelGGL(k_raster_tiled_search_emit, dim3((ni32 + 63) / 64), dim3(64), 0, 0, d_qs.as<WinQuery>(), d_items.as<SearchItem>(), ni32,
                               d_wbits.as<uint32_t>(), d_offs.as<uint64_t>(), to_dev ? out : d_out.as<uint32_t>());
        else
            rc = launch_search_emit(d_qs.as<WinQuery>(), d_items.as<SearchItem>(), ni32, nullptr, d_wbits.as<uint32_t>(), d_offs.as<uint64_t>(),
                                    to_dev ? out : d_out.as<uint32_t>());
        if (rc != DCDF_OK) return rc;
    }
    K2R_HIP(hipEventRecord(ev.e1, 0));
    K2R_HIP(hipGetLastError());
    if (total > 0 && !to_dev) K2R_HIP(hipMemcpy(out, d_out.p, total * 12, hipMemcpyDeviceToHost));
    else K2R_HIP(hipDeviceSynchronize());
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}

// search of dataset-level cubes; vlower / vupper: a value search (lower / upper unused)
static int raster_search(const dcdf_raster* r, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper, const double* vlower,
                         const double* vupper, size_t nq, uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets,
                         float* kernel_ms) {
    const bool value = vlower != nullptr;
    if (r->tiled) {  // elided pieces and has_cells exist in the device pipeline only, which walks k = 2 chunks
        if (!r->all_node || nq > 0x7fffffffu) return DCDF_ERR_UNSUPPORTED;
        return raster_search_device(r, cubes, lower, upper, nq, out, cap, out_mem, counts, offsets, kernel_ms, vlower, vupper);
    }
    // k = 2 chunks: pieces, items, counts, offsets and triples all stay on the device; other arities take the host-built form below
    if (r->all_node && nq <= 0x7fffffffu && !std::getenv("K2R_SEARCH_DFS") && !std::getenv("K2R_RASTER_HOST"))
        return raster_search_device(r, cubes, lower, upper, nq, out, cap, out_mem, counts, offsets, kernel_ms, vlower, vupper);
    std::vector<dcdf_chunk*> sch;
    std::vector<dcdf_cube> scube;
    std::vector<int64_t> slo, shi;
    std::vector<double> svlo, svhi;
    std::vector<uint32_t> sorg, scid, first(nq + 1, 0);
    sch.reserve(2 * nq); scube.reserve(2 * nq); sorg.reserve(6 * nq); scid.reserve(2 * nq);
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > r->T || c.bottom > r->R || c.right > r->C) return DCDF_ERR_BOUNDS;
        if (cube_cells(c) != 0)
            raster_pieces(r, c, [&](uint32_t cid, const dcdf_cube& l, uint32_t t0, uint32_t r0, uint32_t c0) {
                sch.push_back(r->chunks[cid]);
                scid.push_back(cid);
                scube.push_back(l);
                if (value) {
                    svlo.push_back(vlower[q]);
                    svhi.push_back(vupper[q]);
                } else {
                    slo.push_back(lower[q]);
                    shi.push_back(upper[q]);
                }
                sorg.push_back(t0);
                sorg.push_back(r0);
                sorg.push_back(c0);
            });
        first[q + 1] = (uint32_t)sch.size();
    }
    for (size_t q = 0; q < nq; q++) counts[q] = offsets[q] = 0;
    if (sch.empty()) return DCDF_OK;
    std::vector<uint64_t> scnt(sch.size()), soff(sch.size());
    size_t total = 0;
    // the pieces of one query follow each other (segments, then tile rows, then tile columns) and search_impl emits in
    // query order, so a query's triples are contiguous; each is moved to raster coordinates as it is written
    const SearchCtx ctx{&r->d_refs, scid.data(), sorg.data(), r->all_node, r->all_narrow, r->all_wave};
    const int rc = search_impl(sch.data(), scube.data(), value ? nullptr : slo.data(), value ? nullptr : shi.data(), sch.size(), out, cap,
                               scnt.data(), soff.data(), &total, kernel_ms, out_mem, &ctx, value ? svlo.data() : nullptr,
                               value ? svhi.data() : nullptr);
    if (rc != DCDF_OK) return rc;
    for (size_t q = 0; q < nq; q++) {
        offsets[q] = first[q] < sch.size() ? soff[first[q]] : total;
        for (uint32_t k = first[q]; k < first[q + 1]; k++) counts[q] += scnt[k];
    }
    return DCDF_OK;
}
extern "C" int dcdf_raster_search_batch(const dcdf_raster* r, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper, size_t nq,
                                        uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets, float* kernel_ms) {
    if (!r || !cubes || !lower || !upper || !counts || !offsets || nq == 0 || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE) return DCDF_ERR_BAD_ARG;
    return raster_search(r, cubes, lower, upper, nullptr, nullptr, nq, out, cap, out_mem, counts, offsets, kernel_ms);
}
// value search of dataset-level cubes (dcdf_k2r.h): the same routing; k = 2 rasters translate the bounds per piece on the device
extern "C" int dcdf_raster_search_values_batch(const dcdf_raster* r, const dcdf_cube* cubes, const double* lower, const double* upper, size_t nq,
                                               uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets, float* kernel_ms) {
    if (!r || !cubes || !lower || !upper || !counts || !offsets || nq == 0 || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE) return DCDF_ERR_BAD_ARG;
    if (r->bad_fbits) return DCDF_ERR_BAD_ARG;
    for (size_t q = 0; q < nq; q++)
        if (lower[q] != lower[q] || upper[q] != upper[q]) return DCDF_ERR_BAD_ARG;
    return raster_search(r, cubes, nullptr, nullptr, lower, upper, nq, out, cap, out_mem, counts, offsets, kernel_ms);
}

// ---- dataset-level get / fill_cell (Superchunk::get / fill_cell, superchunk.rs:313-400), plain and tiled rasters ----------------
// One thread per point or series element routes to its leaf: an elided leaf's value, or k_get's descent into the chunk at
// (row0 + r, col0 + c); the result is typed by store_typed.  Series: element e belongs to the series s with first[s] <= e <
// first[s + 1] (exclusive prefix of the lengths), found by bisection; its value goes to at[s] + (e - first[s]).
__global__ void __launch_bounds__(256)
k_raster_points(const ChunkRef* __restrict__ refs, const RasterLeaf* __restrict__ leaves, const int64_t* __restrict__ vals, RasterGeom g,
                const uint32_t* __restrict__ q, uint32_t n, const uint64_t* __restrict__ first, uint32_t n_series, const uint64_t* __restrict__ at,
                void* __restrict__ out, int32_t dtype) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    uint32_t t, row, col;
    uint64_t off = e;
    if (first) {
        uint32_t a = 0, b = n_series;  // the last s with first[s] <= e
        while (b - a > 1) {
            const uint32_t m = (a + b) / 2;
            if (first[m] <= e) a = m;
            else b = m;
        }
        const uint32_t* C = q + 4 * (size_t)a;
        t = min(C[0], C[1]) + (uint32_t)(e - first[a]);
        row = C[2];
        col = C[3];
        off = at[a] + (e - first[a]);
    } else {
        t = q[3 * (size_t)e];
        row = q[3 * (size_t)e + 1];
        col = q[3 * (size_t)e + 2];
    }
    const uint32_t seg = t / g.cs, ti = row / g.tile, tj = col / g.tile;
    const uint32_t leaf = (seg * g.nti + ti) * g.ntj + tj, lt = t - seg * g.cs, lr = row - ti * g.tile, lc = col - tj * g.tile;
    if (leaves && leaves[leaf].elided) {
        store_typed(out, (int64_t)off, dtype, vals[(size_t)leaf * g.cs + lt], leaves[leaf].fbits);
        return;
    }
    const uint32_t r0 = leaves ? leaves[leaf].row0 : 0u, c0 = leaves ? leaves[leaf].col0 : 0u;
    const ChunkRef C = refs[leaf];
    store_typed(out, (int64_t)off, dtype, inst_get(C.bytes, C.descs, lt, r0 + lr, c0 + lc), C.fbits);
}
// n elements (points, or series elements of n_series series at first / at); host output is staged densely on the device
static int raster_points(const dcdf_raster* r, const uint32_t* q, size_t nq_words, uint32_t n, const std::vector<uint64_t>* first,
                         const std::vector<uint64_t>* at, uint64_t out_elems, void* out, int32_t out_dtype, int out_mem, float* kernel_ms) {
    const size_t es = elem_size(out_dtype);
    const bool to_dev = out_mem == DCDF_MEM_DEVICE;
    DevBuf d_q, d_first, d_at, d_o;
    K2R_HIP(upload(d_q, q, nq_words * 4));
    const uint32_t n_series = first ? (uint32_t)first->size() : 0u;
    if (first) {
        K2R_HIP(upload(d_first, *first));
        K2R_HIP(upload(d_at, *at));
    }
    if (!to_dev) K2R_HIP(d_o.alloc_pooled(out_elems * es));
    const RasterGeom g{r->T, r->R, r->C, r->tile, r->cs, r->nti, r->ntj, 0u};
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    hipLaunchKernelGGL(k_raster_points, dim3((n + 255) / 256), dim3(256), 0, 0, r->d_refs.as<ChunkRef>(), r->tiled ? r->d_leaf.as<RasterLeaf>() : nullptr,
                       r->tiled ? r->d_vals.as<int64_t>() : nullptr, g, d_q.as<uint32_t>(), n, first ? d_first.as<uint64_t>() : nullptr, n_series,
                       first ? d_at.as<uint64_t>() : nullptr, to_dev ? out : d_o.p, out_dtype);
    K2R_HIP(hipGetLastError());
    K2R_HIP(hipEventRecord(ev.e1, 0));
    if (!to_dev) K2R_HIP(hipMemcpy(out, d_o.p, out_elems * es, hipMemcpyDeviceToHost));
    else K2R_HIP(hipDeviceSynchronize());
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
extern "C" int dcdf_raster_get_batch(const dcdf_raster* r, const uint32_t* points, size_t n, void* out, int32_t out_dtype, int out_mem,
                                     float* kernel_ms) {
    if (!r || !points || !out || n == 0 || n > 0x7fffffffu || !out_args_ok(out_dtype, out_mem)) return DCDF_ERR_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (points[3 * i] >= r->T || points[3 * i + 1] >= r->R || points[3 * i + 2] >= r->C) return DCDF_ERR_BOUNDS;
    return raster_points(r, points, 3 * n, (uint32_t)n, nullptr, nullptr, n, out, out_dtype, out_mem, kernel_ms);
}
extern "C" int dcdf_raster_fill_cell_batch(const dcdf_raster* r, const uint32_t* cells, size_t n, void* out, int32_t out_dtype, int out_mem,
                                           const uint64_t* out_offset, float* kernel_ms) {
    if (!r || !cells || !out || n == 0 || n > 0x7fffffffu || !out_args_ok(out_dtype, out_mem)) return DCDF_ERR_BAD_ARG;
    // the series that hold elements (empty ones write nothing), their first element, and where they go
    std::vector<uint32_t> q;
    std::vector<uint64_t> first, at;
    uint64_t total = 0;
    bool dense = true;
    for (size_t i = 0; i < n; i++) {
        const uint32_t a = std::min(cells[4 * i], cells[4 * i + 1]), b = std::max(cells[4 * i], cells[4 * i + 1]);
        if (b > r->T || cells[4 * i + 2] >= r->R || cells[4 * i + 3] >= r->C) return DCDF_ERR_BOUNDS;
        const uint64_t o = out_offset ? out_offset[i] : total;
        dense = dense && (!out_offset || out_offset[i] == total + out_offset[0]);
        if (b == a) continue;
        q.insert(q.end(), cells + 4 * i, cells + 4 * i + 4);
        first.push_back(total);
        at.push_back(o);
        total += b - a;
    }
    if (total == 0) {
        if (kernel_ms) *kernel_ms = 0.f;
        return DCDF_OK;
    }
    if (total > 0x7fffffffu) return DCDF_ERR_CAPACITY;
    if (out_mem == DCDF_MEM_DEVICE) return raster_points(r, q.data(), q.size(), (uint32_t)total, &first, &at, 0, out, out_dtype, out_mem, kernel_ms);
    // host output: written densely on the device, then moved to the caller's offsets
    const size_t es = elem_size(out_dtype);
    const uint64_t base = out_offset ? out_offset[0] : 0;
    if (dense) return raster_points(r, q.data(), q.size(), (uint32_t)total, &first, &first, total, (uint8_t*)out + base * es, out_dtype, out_mem, kernel_ms);
    std::vector<uint8_t> tmp(total * es);
    const int rc = raster_points(r, q.data(), q.size(), (uint32_t)total, &first, &first, total, tmp.data(), out_dtype, out_mem, kernel_ms);
    if (rc != DCDF_OK) return rc;
    for (size_t s = 0; s < first.size(); s++) {
        const uint64_t len = (s + 1 < first.size() ? first[s + 1] : total) - first[s];
        std::memcpy((uint8_t*)out + at[s] * es, tmp.data() + first[s] * es, len * es);
    }
    return DCDF_OK;
}