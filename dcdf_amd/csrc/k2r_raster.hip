// k2r_raster.hip -- C ABI, query side: a tiled, time-segmented raster of opened chunks (dcdf_raster_*): the handle and its two
// constructors, fill_window, search, get / fill_cell.  Routes dataset-level cubes and points to their chunks on the device and runs
// the walks of k2r_query.hip over the pieces.  The calls that read whole regions are k2r_raster_region.hip's.
#include <hip/hip_runtime.h>

#include <new>

#include "k2r_raster_host.h"

using namespace k2r;

// ---- a tiled, time-segmented raster of opened chunks: the routing of the layers above, natively ---------------------------------
// Variable::append cuts [instants, rows, cols] into time segments of chunk_size instants (dataset.rs:838) and Superchunk::build
// cuts each segment into tile x tile sub-arrays (superchunk.rs:127-181); reads are routed back the same way (Span::fill_window
// span.rs:190-216 over time, Superchunk::subchunks_for superchunk.rs:589-633 over rows / cols).  dcdf_raster does that split for a
// whole batch of dataset-level cubes on the host in C++ and decodes every piece in ONE launch straight into its place in the
// caller's window (the pieces carry the parent window's strides): no per-piece copies, no reassembly, the chunk table uploaded once.
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
    r->plan_leaves.assign(n, PlanLeaf{});
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
// chunk h is leaf i, which starts at (row0, col0) of it
static void raster_add_chunk(dcdf_raster* r, RasterTables& t, size_t i, dcdf_chunk* h, uint32_t row0 = 0, uint32_t col0 = 0) {
    r->chunks[i] = h;
    r->plan_leaves[i] = PlanLeaf{row0, col0, h->encoding, h->fbits, 0, (uint8_t)(h->top_g && h->narrow32)};
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
            r->plan_leaves[i] = PlanLeaf{0, 0, f.enc, f.fbits, 1, 0};  // (RasterLeaf's, as the device reads them)
            continue;
        }
        // the chunk must cover the leaf at (row0, col0), with the leaf's instants
        if (h->instants != li || (uint64_t)L.row0 + lr > h->rows || (uint64_t)L.col0 + lc > h->cols) return DCDF_ERR_BAD_ARG;
        f.row0 = L.row0;
        f.col0 = L.col0;
        raster_add_chunk(r.get(), t, i, h, L.row0, L.col0);
    }
    rc = raster_upload(r.get(), t);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(upload(r->d_leaf, r->leaves));
    K2R_HIP(upload(r->d_vals, vals));
    K2R_HIP(upload(r->d_mm, mm));
    *out = r.release();
    return DCDF_OK;
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
    auto along = [&](uint32_t a, uint32_t b, uint32_t unit) {  // axis_items summed over the tiles [a, b) meets
        uint64_t n = 0;
        for (uint32_t t = a / unit; t <= (b - 1) / unit; t++) n += axis_items(std::max(a, t * unit) - t * unit, std::min(b, t * unit + unit) - t * unit, step);
        return n;
    };
    return (uint64_t)(c.end - c.start) * along(c.top, c.bottom, r->tile) * along(c.left, c.right, r->tile);
}

// ---- tiled rasters: fill_window -------------------------------------------------------------------------------------------
// A piece on a chunk leaf is decoded by the wave walk at (row0 + r, col0 + c) of its chunk; a piece on an elided leaf becomes a
// ConstPiece (k2r_plan.h): one value per instant over a rectangle of the window, written by k_raster_fill_const in the same call.
// wave items and constant pieces of one cube of a tiled raster
static void tiled_item_count(const dcdf_raster* r, const dcdf_cube& c, uint32_t step, uint64_t* n_items, uint64_t* n_const) {
    raster_pieces(r->plan(), c, [&](uint32_t cid, const dcdf_cube& l, uint32_t, uint32_t, uint32_t) {
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
int k2r::launch_raster_fill_const(const dcdf_raster* r, const ConstPiece* d_consts, uint32_t n, void* d_out, int32_t out_dtype) {
    if (n == 0) return DCDF_OK;
    hipLaunchKernelGGL(k_raster_fill_const, dim3(std::min(n, 256u * 64u)), dim3(256), 0, 0, d_consts, n, r->d_leaf.as<RasterLeaf>(), r->d_vals.as<int64_t>(),
                       r->cs, d_out, out_dtype);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
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
        rc = launch_raster_fill_const(r, d_consts.as<ConstPiece>(), (uint32_t)n_const, W.dst(), out_dtype);
        if (rc != DCDF_OK) return rc;
        if (n_items)
            rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>(), (uint32_t)n_items, W.dst(), out_dtype, nullptr, ev.e1, r->all_node,
                                         r->all_narrow);
    }
    if (rc != DCDF_OK) return rc;
    return batch_epilogue(W, ev, r->tiled && n_items == 0, kernel_ms);
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
            raster_pieces(r->plan(), c, [&](uint32_t cid, const dcdf_cube& l, uint32_t t0, uint32_t r0, uint32_t c0) {
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