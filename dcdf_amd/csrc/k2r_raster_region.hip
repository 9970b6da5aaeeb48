// k2r_raster_region.hip -- C ABI, query side: the calls that read whole regions of a raster -- decode, reduce over time (plain and grouped), moments
// over time (plain and grouped), spell statistics, quantiles over time, regression over time (plain and grouped), rolling windows over time (plain and grouped), reduce over space, histogram, zonal statistics -- with their fold / finish kernels.  The plan of every call is host code of its own (k2r_plan.h); here
// are the arguments, the uploads and the launches.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "k2r_moment.h"
#include "k2r_raster_host.h"
#include "k2r_regress.h"
#include "k2r_rolling.h"

using namespace k2r;

// ---- what the ten calls share -----------------------------------------------------------------------------------------------
// Arguments (own_args_ok: the call's own), support, the zero state of the two reports, the cubes' bounds -- in the order of the
// error codes.  EXACT_FLOATS: the call's arithmetic takes no float chunk with fractional bits value_bounds refuses.
enum RegionFloats { ANY_FLOATS, EXACT_FLOATS };
static int region_begin(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const void* out, const uint64_t* out_offset, int out_mem,
                        bool own_args_ok, RegionFloats floats, uint64_t stats[3], float* kernel_ms) {
    if (!r || !cubes || !out || !out_offset || nq > 0x7fffffffu || !own_args_ok || (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE))
        return DCDF_ERR_BAD_ARG;
    if (!r->all_wave || (floats == EXACT_FLOATS && r->bad_fbits)) return DCDF_ERR_UNSUPPORTED;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (kernel_ms) *kernel_ms = 0.f;
    return plan_bounds(r->plan(), cubes, nq);
}
static void put_stats(uint64_t stats[3], const uint64_t cells[3]) {
    if (stats)
        for (int i = 0; i < 3; i++) stats[i] = cells[i];
}
template <class T>
static int upload_some(DevBuf& d, const std::vector<T>& v) {
    if (!v.empty()) K2R_HIP(upload(d, v));
    return DCDF_OK;
}
// A cap a test may override through the environment (read on every call: the tests change it between calls of one process).
static uint64_t env_cap(const char* name, uint64_t dflt) {
    const char* e = std::getenv(name);
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : dflt;
}
static uint64_t reduce_slab_cells() { return env_cap("K2R_REDUCE_SLAB_CELLS", (uint64_t)1 << 22); }  // cells of one fallback slab
static uint64_t space_record_cap() { return env_cap("K2R_SPACE_RECORDS", (uint64_t)6 << 20); }      // records of a batch, 40 bytes each
static uint64_t zonal_acc_cap() { return env_cap("K2R_ZONAL_ACC_BYTES", (uint64_t)128 << 20); }     // 72 bytes per (zone, instant)
static uint64_t quantile_slab_bytes() { return env_cap("K2R_QUANTILE_SLAB_BYTES", (uint64_t)256 << 20); }  // stored integers of one band
// A fold kernel over n pieces on the null stream: a column of gy workgroups per piece.
template <auto Kernel, class Fold, class... Args>
static int launch_fold(uint32_t gy, const Fold* d_ps, size_t n, Args... args) {
    if (n == 0) return DCDF_OK;
    hipLaunchKernelGGL(Kernel, dim3((uint32_t)std::min<size_t>(n, 1u << 20), gy), dim3(256), 0, 0, d_ps, (uint32_t)n, args...);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}
// the window walk's share of a plan on the device: its items, its folds, and the slab both kinds of launch meet in
struct WalkDev {
    DevBuf items, folds, slab;
    template <class Fold>
    int upload(const SlabCutter<Fold>& w) {
        int rc = upload_some(items, w.items);
        if (rc == DCDF_OK) rc = upload_some(folds, w.folds);
        if (rc == DCDF_OK && w.slab_max) K2R_HIP(slab.alloc_pooled(w.slab_max * sizeof(int64_t)));
        return rc;
    }
    // the slabs [s0, s1) one after the other: the walk decodes a slab's items as stored integers (DCDF_I64: store_typed leaves n
    // as it is) -- one launch whatever mix of encodings its chunks have --, then the call's fold kernel reads the slab
    template <auto Kernel, class Fold, class... Args>
    int run(const dcdf_raster* r, const SlabCutter<Fold>& w, const PlanRange& g, uint32_t gy, Args... args) const {
        for (size_t s = g.slab0; s < g.slab1; s++) {
            const Slab& b = w.slabs[s];
            int rc = launch_window_items_dev(r->d_refs, items.as<WinItem>() + b.item0, (uint32_t)(b.item1 - b.item0), slab.p, DCDF_I64, nullptr, nullptr,
                                             r->all_node, r->all_narrow);
            if (rc == DCDF_OK) rc = launch_fold<Kernel>(gy, folds.as<Fold>() + b.fold0, b.fold1 - b.fold0, slab.as<int64_t>(), nullptr, args...);
            if (rc != DCDF_OK) return rc;
        }
        return DCDF_OK;
    }
};
// One array of T per cube -- the masks of reduce_space and histogram (optional: a null array stages nothing), the labels of zonal
// (mandatory; their pooled copy holds at least one element: MIN).  Cube q's elements start at p[moff[q]] -- in the caller's device
// array, or in a pooled copy of the host arrays of the cubes that have instants, one after the other (stage()).
template <class T, uint64_t MIN>
struct CubeArrays {
    std::vector<uint64_t> moff;
    uint64_t total = 0;
    const T* p;
    bool host;
    DevBuf d_copy;
    static bool args_ok(const T* a, const uint64_t* offset, int mem) { return !a || (offset && (mem == DCDF_MEM_HOST || mem == DCDF_MEM_DEVICE)); }
    CubeArrays(const dcdf_cube* cubes, size_t nq, const T* a, const uint64_t* offset, int mem) : moff(nq, 0), p(a), host(a && mem == DCDF_MEM_HOST) {
        for (size_t q = 0; a && q < nq; q++) {
            const dcdf_cube c = norm_cube(cubes[q]);
            if (c.end == c.start) continue;
            moff[q] = host ? total : offset[q];
            total += (uint64_t)(c.bottom - c.top) * (c.right - c.left);
        }
    }
    int stage(const dcdf_cube* cubes, size_t nq, const uint64_t* offset) {
        if (!host) return DCDF_OK;
        K2R_HIP(d_copy.alloc_pooled(std::max<uint64_t>(total, MIN) * sizeof(T)));
        for (size_t q = 0; q < nq; q++) {
            const dcdf_cube c = norm_cube(cubes[q]);
            const uint64_t n = (uint64_t)(c.bottom - c.top) * (c.right - c.left);
            if (c.end == c.start || n == 0) continue;
            K2R_HIP(hipMemcpy((T*)d_copy.p + moff[q], p + offset[q], n * sizeof(T), hipMemcpyHostToDevice));
        }
        p = (const T*)d_copy.p;
        return DCDF_OK;
    }
};
using CubeMasks = CubeArrays<uint8_t, 0>;
using CubeLabels = CubeArrays<uint16_t, 1>;
// Where the planes of reduce_time and spells go: cube q's output is n_out "instants" of [rows][cols] to WindowOut, its n_scr
// scratch planes start at element sbase[q] of a pooled array of scr_total elements.
struct PlaneLayout {
    std::vector<dcdf_cube> planes;
    std::vector<uint64_t> sbase;
    uint64_t scr_total = 0;
    PlaneLayout(const dcdf_cube* cubes, size_t nq, uint32_t n_out, uint32_t n_scr) : planes(nq, dcdf_cube{}), sbase(nq, 0) {
        for (size_t q = 0; q < nq; q++) {
            const dcdf_cube c = norm_cube(cubes[q]);
            if (cube_cells(c) == 0) continue;
            planes[q] = dcdf_cube{0, n_out, c.top, c.bottom, c.left, c.right};
            sbase[q] = scr_total;
            scr_total += (uint64_t)n_scr * (c.bottom - c.top) * (c.right - c.left);
        }
    }
};
// What follows a successful plan in reduce_time, spells, reduce_space and zonal (decode and histogram keep their own lines, see
// DESIGN.md "Speed"), in this order (a call's own allocations and uploads go between the steps):
// begin -- the stats out; `nothing` when no cell is written, else the host form's stage --, upload, start -- the events, e0
// recorded --, the launches, end (batch_epilogue).
struct RegionRun {
    DevBuf units, cfolds;
    WalkDev walk;
    EventPair ev;
    bool nothing = false;
    int begin(WindowOut& W, uint64_t stats[3], const uint64_t cells[3]) {
        put_stats(stats, cells);
        nothing = W.total == 0;
        if (!nothing && !W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
        return DCDF_OK;
    }
    template <class Plan>
    int upload(const Plan& P) {
        int rc = upload_some(units, P.units);
        if (rc == DCDF_OK) rc = upload_some(cfolds, P.cfolds);
        return rc == DCDF_OK ? walk.upload(P.walk) : rc;
    }
    int start() {
        K2R_HIP(ev.create());
        K2R_HIP(hipEventRecord(ev.e0, 0));
        return DCDF_OK;
    }
    // the elided pieces of range g, one value per instant from dcdf_raster::d_vals (the range's slabs: walk.run)
    template <auto Kernel, class Fold, class... Args>
    int fold_consts(const dcdf_raster* r, const PlanRange& g, uint32_t gy, Args... args) const {
        return launch_fold<Kernel>(gy, cfolds.as<Fold>() + g.const0, g.const1 - g.const0, nullptr, r->d_vals.as<int64_t>(), args...);
    }
    int end(const WindowOut& W, bool record, float* kernel_ms) const { return batch_epilogue(W, ev, record, kernel_ms); }
};

// ---- decompress: whole regions, block by block (k2r_bulk.hip) ---------------------------------------------------------------
// plan_decode (k2r_plan.h): BulkUnits for the pieces on chunks the bulk kernel takes, the wave items dcdf_raster_fill_window_batch
// makes of the pieces on any other chunk, a ConstPiece per elided piece.  All three write the same output array.
extern "C" int dcdf_raster_decode_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype, int out_mem,
                                        const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, out_args_ok(out_dtype, out_mem), ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    WindowOut W(cubes, nq, out, out_offset, elem_size(out_dtype), out_mem == DCDF_MEM_DEVICE);
    DecodePlan P;
    rc = plan_decode(r->plan(), cubes, nq, W.base.data(), r->all_node, bulk_wanted_units(), P);
    if (rc != DCDF_OK) return rc;
    put_stats(stats, P.stats);
    if (W.total == 0) return DCDF_OK;
    DevBuf d_units, d_consts, d_items;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    void* const d_out = W.dst();
    rc = upload_some(d_units, P.units);
    if (rc == DCDF_OK) rc = upload_some(d_consts, P.consts);
    if (rc == DCDF_OK) rc = upload_some(d_items, P.items);
    if (rc != DCDF_OK) return rc;
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    rc = launch_raster_fill_const(r, d_consts.as<ConstPiece>(), (uint32_t)P.consts.size(), d_out, out_dtype);
    if (rc == DCDF_OK) rc = launch_bulk_decode(r->d_refs.as<ChunkRef>(), d_units.as<BulkUnit>(), (uint32_t)P.units.size(), d_out, out_dtype);
    if (rc == DCDF_OK && !P.items.empty())
        rc = launch_window_items_dev(r->d_refs, d_items.as<WinItem>(), (uint32_t)P.items.size(), d_out, out_dtype, nullptr, ev.e1, r->all_node,
                                     r->all_narrow);
    if (rc != DCDF_OK) return rc;
    return batch_epilogue(W, ev, P.items.empty(), kernel_ms);
}
// ---- per-cell folds over time: reduce_time, reduce_time_groups, moments_time and spells (k2r_cell_fold.h) ---------------------
// The plan, and what keeps a cell's instants in order, are plan_reduce_time's and plan_spells' (k2r_plan.h): the segments are
// launched one after the other in ascending order on the null stream, and every piece continues the state its cells' planes
// hold.  The state planes are the output planes themselves (cube q's requested planes in ascending bit order); states kept for
// another's sake alone live in pooled scratch planes (state_plane).
//
// Pieces on chunks the bulk kernel does not take are decoded by the window walk as stored integers (DCDF_I64: store_typed
// leaves n as it is) into a slab of a bounded number of cells -- one walk launch per slab whatever mix of encodings its chunks
// have --, then folded by k_cell_fold: a thread per cell, its instants in order.  Elided pieces are folded by the same kernel
// straight from dcdf_raster::d_vals (one value per instant).  Op -- a per-cell statistic -- has
//   Piece, T                 the fold record, a CellFold (k2r_cell_fold.h) and what else the statistic needs; the planes' element
//   Op(P, dst, scr, ops, x...)  per piece: the plane pointers; x: what else the statistic's kernel is given (X)
//   init() / load(at)        the cell's initial state / its state from the planes (only when the piece continues a cube)
//   step(P, t, n)            the stored integer n of the piece's instant t into the state
//   store(at)                the state into the planes
template <class Op, class... X>
__global__ void __launch_bounds__(256)
k_cell_fold(const typename Op::Piece* __restrict__ ps, uint32_t n, const int64_t* __restrict__ slab, const int64_t* __restrict__ vals,
            typename Op::T* dst, typename Op::T* scr, uint32_t ops, X... x) {
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const typename Op::Piece P = ps[p];
        const uint64_t cells = (uint64_t)P.rows * P.cols;
        Op op(P, dst, scr, ops, x...);
        for (uint64_t e = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; e < cells; e += (uint64_t)gridDim.y * blockDim.x) {
            const uint64_t at = e / P.cols * P.sr + e % P.cols;
            op.init();
            if (!P.init) op.load(at);
            for (uint32_t t = 0; t < P.nt; t++) op.step(P, t, P.elided ? vals[P.src + t] : slab[P.src + (uint64_t)t * cells + e]);
            op.store(at);
        }
    }
}
// reduce_time (k2r_reduce.h): the leaf's own encoding applied to the stored integer (reduce_widen: the conversions of
// store_typed, so the value is the typed fill_window's), then the four accumulators as doubles
struct ReduceCell {
    typedef FoldPiece Piece;
    typedef double T;
    const uint32_t live;
    double *const p_min, *const p_max, *const p_sum, *const p_cnt;
    double s, c, lo, hi;
    __device__ ReduceCell(const FoldPiece& P, double* dst, double* scr, uint32_t ops)
        : live(reduce_live(ops)),
          p_min(reduce_plane(RA_MIN, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_max(reduce_plane(RA_MAX, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_sum(reduce_plane(RA_SUM, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_cnt(reduce_plane(RA_COUNT, dst, scr, ops, P.o_off, P.s_off, P.psz)) {}
    __device__ void init() {
        s = c = 0.0;
        lo = hi = __builtin_nan("");
    }
    __device__ void load(uint64_t at) {
        if (live & RA_MIN) lo = p_min[at];
        if (live & RA_MAX) hi = p_max[at];
        if (live & RA_SUM) s = p_sum[at];
        if (live & RA_COUNT) c = p_cnt[at];
    }
    __device__ void step(const FoldPiece& P, uint32_t, int64_t n) {
        const double x = reduce_widen(P.enc, P.fbits, n);
        if (x == x) {
            s = s + x;
            c = c + 1.0;
            lo = fmin(lo, x);
            hi = fmax(hi, x);
        }
    }
    __device__ void store(uint64_t at) const {
        if (live & RA_MIN) p_min[at] = lo;
        if (live & RA_MAX) p_max[at] = hi;
        if (live & RA_SUM) p_sum[at] = s;
        if (live & RA_COUNT) p_cnt[at] = c;
    }
};
// spells (k2r_spell.h): spell_step, the hit test on the stored integer itself
struct SpellCell {
    typedef SpellFold Piece;
    typedef uint32_t T;
    const uint32_t live;
    uint32_t *const p_cnt, *const p_lng, *const p_lst, *const p_fst, *const p_las, *const p_cur;
    SpellState s;
    __device__ SpellCell(const SpellFold& P, uint32_t* dst, uint32_t* scr, uint32_t ops)
        : live(spell_live(ops)),
          p_cnt(spell_plane(SP_COUNT, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_lng(spell_plane(SP_LONGEST, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_lst(spell_plane(SP_LSTART, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_fst(spell_plane(SP_FIRST, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_las(spell_plane(SP_LAST, dst, scr, ops, P.o_off, P.s_off, P.psz)),
          p_cur(spell_plane(SP_CUR, dst, scr, ops, P.o_off, P.s_off, P.psz)) {}
    __device__ void init() { s = spell_init(); }
    __device__ void load(uint64_t at) {
        if (live & SP_COUNT) s.count = p_cnt[at];
        if (live & SP_LONGEST) s.longest = p_lng[at];
        if (live & SP_LSTART) s.lstart = p_lst[at];
        if (live & SP_FIRST) s.first = p_fst[at];
        if (live & SP_LAST) s.last = p_las[at];
        if (live & SP_CUR) s.cur = p_cur[at];
    }
    __device__ void step(const SpellFold& P, uint32_t t, int64_t v) {
        if (P.enc == ENC_I32) v = (int64_t)(int32_t)v;  // (store_typed's conversion)
        spell_step(s, P.dt + t, spell_hit64(v, P.lo, P.hi, P.flags));
    }
    __device__ void store(uint64_t at) const {
        if (live & SP_COUNT) p_cnt[at] = s.count;
        if (live & SP_LONGEST) p_lng[at] = s.longest;
        if (live & SP_LSTART) p_lst[at] = s.lstart;
        if (live & SP_FIRST) p_fst[at] = s.first;
        if (live & SP_LAST) p_las[at] = s.last;
        if (live & SP_CUR) p_cur[at] = s.cur;
    }
};
// reduce_time_groups (k2r_group.h): ReduceCell's accumulators for one run of equal labels at a time (group_step), merged into
// the run's group at a change of group and at the piece's end.  A GroupFold never initialises -- the planes are filled first --,
// so load() always runs: it is where the cell's planes are taken.
struct GroupCell {
    typedef GroupFold Piece;
    typedef double T;
    const uint16_t* const labels;
    const uint32_t n_groups;
    GroupPlanes base, at;  // of the piece's first cell, of the thread's cell
    GroupState st;
    __device__ GroupCell(const GroupFold& P, double* dst, double* scr, uint32_t ops, const uint16_t* labels_, uint32_t n_groups_)
        : labels(labels_ + P.lab), n_groups(n_groups_) {
        const uint32_t live = reduce_live(ops);
        base.p_min = live & RA_MIN ? reduce_plane(RA_MIN, dst, scr, ops, P.o_off, P.s_off, P.psz) : nullptr;
        base.p_max = live & RA_MAX ? reduce_plane(RA_MAX, dst, scr, ops, P.o_off, P.s_off, P.psz) : nullptr;
        base.p_sum = live & RA_SUM ? reduce_plane(RA_SUM, dst, scr, ops, P.o_off, P.s_off, P.psz) : nullptr;
        base.p_cnt = live & RA_COUNT ? reduce_plane(RA_COUNT, dst, scr, ops, P.o_off, P.s_off, P.psz) : nullptr;
        base.gsz = P.gsz;
        at = base;
    }
    __device__ void init() { st = group_init(); }
    __device__ void load(uint64_t e) {
        at.p_min = base.p_min ? base.p_min + e : nullptr;
        at.p_max = base.p_max ? base.p_max + e : nullptr;
        at.p_sum = base.p_sum ? base.p_sum + e : nullptr;
        at.p_cnt = base.p_cnt ? base.p_cnt + e : nullptr;
    }
    __device__ void step(const GroupFold& P, uint32_t t, int64_t n) { group_step(st, at, labels[t], n_groups, reduce_widen(P.enc, P.fbits, n)); }
    __device__ void store(uint64_t) const { group_merge(st, at); }
};
// the identities of every live accumulator of reduce_time_groups into the cubes' arrays, before the first segment: SUM 0.0,
// COUNT 0, MIN / MAX NaN.  A group no instant belongs to keeps them (and MEAN's 0 / 0 case makes its NaN).
__global__ void __launch_bounds__(256) k_group_fill(const MeanPiece* __restrict__ ps, uint32_t n, double* dst, double* scr, uint32_t ops) {
    const uint32_t live = reduce_live(ops);
    for (uint32_t p = blockIdx.y; p < n; p += gridDim.y) {
        const MeanPiece P = ps[p];
        for (uint32_t A = RA_MIN; A <= RA_COUNT; A <<= 1) {
            if (!(live & A)) continue;
            double* const q = reduce_plane(A, dst, scr, ops, P.o_off, P.s_off, P.psz);
            const double v = A & (RA_MIN | RA_MAX) ? __builtin_nan("") : 0.0;
            for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < P.psz; e += (uint64_t)gridDim.x * blockDim.x) q[e] = v;
        }
    }
}
// moments_time / moments_time_groups (k2r_moment.h): the state (c, K, s1, s2) of one run of equal labels at a time
// (moment_group_step), stored whole at a change of group and at the piece's end.  As GroupCell: the planes are filled first, no
// piece initialises, load() is where the cell's planes are taken.  Without a label array every instant is group 0.
struct MomentCell {
    typedef GroupFold Piece;
    typedef double T;
    const uint16_t* const labels;
    const uint32_t n_groups;
    MomentPlanes base, at;  // of the piece's first cell, of the thread's cell
    MomentRun st;
    __device__ MomentCell(const GroupFold& P, double* dst, double* scr, uint32_t ops, const uint16_t* labels_, uint32_t n_groups_)
        : labels(labels_ ? labels_ + P.lab : nullptr), n_groups(n_groups_), base(moment_planes(dst, scr, ops, P.o_off, P.s_off, P.psz, P.gsz)), at(base) {}
    __device__ void init() { st = moment_run_init(); }
    __device__ void load(uint64_t e) { at = MomentPlanes{base.p_c + e, base.p_k + e, base.p_s1 + e, base.p_s2 + e, base.gsz}; }
    __device__ void step(const GroupFold& P, uint32_t t, int64_t n) {
        moment_group_step(st, at, moment_label(labels, t), n_groups, reduce_widen(P.enc, P.fbits, n));
    }
    __device__ void store(uint64_t) const { moment_store(st, at); }
};
// the initial state (0, NaN, +0.0, +0.0) into the four state arrays of every cube, before the first segment
__global__ void __launch_bounds__(256) k_moment_fill(const MeanPiece* __restrict__ ps, uint32_t n, double* dst, double* scr, uint32_t ops) {
    const MomentState s0 = moment_init();
    for (uint32_t p = blockIdx.y; p < n; p += gridDim.y) {
        const MeanPiece P = ps[p];
        const MomentPlanes Q = moment_planes(dst, scr, ops, P.o_off, P.s_off, P.psz, 0);
        for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < P.psz; e += (uint64_t)gridDim.x * blockDim.x) {
            Q.p_c[e] = s0.c;
            Q.p_k[e] = s0.K;
            Q.p_s1[e] = s0.s1;
            Q.p_s2[e] = s0.s2;
        }
    }
}
// the finishing kernel of the moments: every cell's (and group's) state into the requested planes of MEAN, VAR and STD
// (moment_finish); COUNT's plane is its state
__global__ void __launch_bounds__(256) k_moment_finish(const MeanPiece* __restrict__ ps, uint32_t n, double* dst, double* scr, uint32_t ops, uint32_t ddof) {
    for (uint32_t p = blockIdx.y; p < n; p += gridDim.y) {
        const MeanPiece P = ps[p];
        const MomentPlanes Q = moment_planes(dst, scr, ops, P.o_off, P.s_off, P.psz, 0);
        double* const p_mean = moment_plane(MO_MEAN, dst, scr, ops, P.o_off, P.s_off, P.psz);
        double* const p_var = moment_plane(MO_VAR, dst, scr, ops, P.o_off, P.s_off, P.psz);
        double* const p_std = moment_plane(MO_STD, dst, scr, ops, P.o_off, P.s_off, P.psz);
        for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < P.psz; e += (uint64_t)gridDim.x * blockDim.x) {
            double o[4];
            moment_finish(MomentState{Q.p_c[e], Q.p_k[e], Q.p_s1[e], Q.p_s2[e]}, ddof, o);
            if (ops & MO_MEAN) p_mean[e] = o[1];
            if (ops & MO_VAR) p_var[e] = o[2];
            if (ops & MO_STD) p_std[e] = o[3];
        }
    }
}
// the finishing kernel of reduce_time: MEAN = SUM / COUNT, NaN where nothing was counted
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
// A kernel over the cubes' arrays of a plan (P.means), a row of workgroups per cube: the fills and the finishing kernels.
template <auto Kernel, class... Args>
static int launch_over_means(const DevBuf& d_means, const std::vector<MeanPiece>& means, Args... args) {
    if (means.empty()) return DCDF_OK;
    uint64_t big = 0;
    for (const MeanPiece& m : means) big = std::max(big, m.psz);
    hipLaunchKernelGGL(Kernel, dim3((uint32_t)std::min<uint64_t>((big + 255) / 256, 2048), (uint32_t)std::min<size_t>(means.size(), 65535)), dim3(256), 0, 0,
                       d_means.as<MeanPiece>(), (uint32_t)means.size(), args...);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}
// What a call hands to cell_fold_batch: the raster, the cubes, `ops`, and its own steps -- make_plan(P, base, sbase) fills the Plan
// (a SegmentPlan), bulk(units, g, d_dst, d_scr) launches the bulk kernel over range g's units -- and, where it needs them, its own
//   staged(P)                     uploads what else the call's launches read, before the events
//   first(P, d_dst, d_scr)        launches what precedes the first segment
//   finish(P, d_dst, d_scr)       launches what follows the last segment
template <class Plan_, class T>
struct CellFoldCall {
    typedef Plan_ Plan;
    const dcdf_raster* r;
    const dcdf_cube* cubes;
    size_t nq;
    uint32_t ops;
    int staged(const Plan&) { return DCDF_OK; }
    int first(const Plan&, T*, T*) { return DCDF_OK; }
    int finish(const Plan&, T*, T*) { return DCDF_OK; }
};
// What follows region_begin in the five calls.  live: the states the call carries, `ops` and those kept for another's sake.
// depth: the [rows][cols] planes of one state (the grouped calls: their groups); x: what k_cell_fold hands to Op besides the
// planes.  Per segment: the elided folds, the bulk units, the walk's slabs -- a segment's pieces share no cell.
template <class Op, class Call, class... X>
static int cell_fold_batch(Call& call, uint32_t live, uint32_t depth, typename Op::T* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                           float* kernel_ms, X... x) {
    typedef typename Op::T T;
    const uint32_t ops = call.ops;
    const PlaneLayout L(call.cubes, call.nq, popc32(ops) * depth, popc32(live & ~ops) * depth);
    WindowOut W(L.planes.data(), call.nq, out, out_offset, sizeof(T), out_mem == DCDF_MEM_DEVICE);
    typename Call::Plan P(reduce_slab_cells());
    int rc = call.make_plan(P, W.base.data(), L.sbase.data());
    if (rc != DCDF_OK) return rc;
    DevBuf d_scr;
    RegionRun R;
    rc = R.begin(W, stats, P.stats);
    if (rc != DCDF_OK || R.nothing) return rc;
    T* const d_dst = (T*)W.dst();
    if (L.scr_total) K2R_HIP(d_scr.alloc_pooled(L.scr_total * sizeof(T)));
    rc = R.upload(P);
    if (rc == DCDF_OK) rc = call.staged(P);
    if (rc == DCDF_OK) rc = R.start();
    if (rc == DCDF_OK) rc = call.first(P, d_dst, d_scr.as<T>());
    if (rc != DCDF_OK) return rc;
    for (const SegRange& g : P.ranges) {
        rc = R.fold_consts<k_cell_fold<Op, X...>, typename Op::Piece>(call.r, g, 16, d_dst, d_scr.as<T>(), ops, x...);
        if (rc == DCDF_OK) rc = call.bulk(R.units, g, d_dst, d_scr.as<T>());
        if (rc == DCDF_OK) rc = R.walk.run<k_cell_fold<Op, X...>>(call.r, P.walk, g, 16, d_dst, d_scr.as<T>(), ops, x...);
        if (rc != DCDF_OK) return rc;
    }
    rc = call.finish(P, d_dst, d_scr.as<T>());
    return rc == DCDF_OK ? R.end(W, true, kernel_ms) : rc;
}
// per-cell min / max / sum / count / mean of the values decode returns (k2r_reduce.h); SUM / COUNT kept for MEAN alone: scratch planes
struct ReduceTimeCall : CellFoldCall<TimePlan, double> {
    DevBuf d_means;
    int make_plan(TimePlan& P, const uint64_t* base, const uint64_t* sbase) { return plan_reduce_time(r->plan(), cubes, nq, base, sbase, r->all_node, P); }
    int bulk(const DevBuf& units, const SegRange& g, double* d_dst, double* d_scr) {
        return launch_bulk_reduce(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), units.as<ReduceUnit>() + g.unit0, (uint32_t)(g.unit1 - g.unit0), d_dst,
                                  d_scr, ops);
    }
    int staged(const TimePlan& P) { return ops & ROP_MEAN ? upload_some(d_means, P.means) : (int)DCDF_OK; }
    int finish(const TimePlan& P, double* d_dst, double* d_scr) {
        return ops & ROP_MEAN ? launch_over_means<k_reduce_mean>(d_means, P.means, d_dst, d_scr, ops) : (int)DCDF_OK;
    }
};
extern "C" int dcdf_raster_reduce_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, double* out, int out_mem,
                                             const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, ops != 0 && ops <= (RA_ALL | ROP_MEAN), ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    ReduceTimeCall call{{r, cubes, nq, ops}};
    return cell_fold_batch<ReduceCell>(call, reduce_live(ops), 1, out, out_mem, out_offset, stats, kernel_ms);
}
// ---- the grouped folds: reduce_time_groups, moments_time and moments_time_groups ----------------------------------------------
// One path: the grouped reduce's plan (plan_reduce_time_groups) and records; the arrays [n_groups][rows][cols] of every state
// filled before the first segment, so every piece continues what the planes hold; a finishing kernel behind the last.
// The device label array (gather_time_labels, k2r_plan.h): allocated before the plan -- its address is a launch argument --,
// copied in one piece in the staged step.  Labels given, yet no cube has cells: nothing is planned and dev() is never read.
struct TimeLabels {
    std::vector<uint64_t> loff;
    std::vector<uint16_t> lab;
    DevBuf d_copy;
    int alloc(const dcdf_cube* cubes, size_t nq, const uint16_t* labels, const uint64_t* label_offset) {
        gather_time_labels(cubes, nq, labels, label_offset, loff, lab);
        if (!lab.empty()) K2R_HIP(d_copy.alloc_pooled(lab.size() * sizeof(uint16_t)));
        return DCDF_OK;
    }
    const uint16_t* dev() const { return lab.empty() ? nullptr : d_copy.as<uint16_t>(); }
    int copy() const {
        if (!lab.empty()) K2R_HIP(hipMemcpy(d_copy.p, lab.data(), lab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        return DCDF_OK;
    }
};
// Bulk: the statistic's bulk launcher; Fill: the kernel of its states' identities, over P.means whatever `ops`; finishing(d_means,
// means, d_dst, d_scr): what makes the planes that are no state.
template <auto Bulk, auto Fill, class Finish>
struct GroupedCall : CellFoldCall<GroupPlan, double> {
    uint32_t n_groups;
    Finish finishing;
    TimeLabels labels;
    DevBuf d_means;
    int make_plan(GroupPlan& P, const uint64_t* base, const uint64_t* sbase) {
        return plan_reduce_time_groups(r->plan(), cubes, nq, labels.loff.data(), n_groups, base, sbase, r->all_node, P);
    }
    int bulk(const DevBuf& units, const SegRange& g, double* d_dst, double* d_scr) {
        return Bulk(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), units.as<GroupUnit>() + g.unit0, (uint32_t)(g.unit1 - g.unit0), labels.dev(), n_groups,
                    d_dst, d_scr, ops);
    }
    int staged(const GroupPlan& P) {
        const int rc = labels.copy();
        return rc == DCDF_OK ? upload_some(d_means, P.means) : rc;
    }
    int first(const GroupPlan& P, double* d_dst, double* d_scr) { return launch_over_means<Fill>(d_means, P.means, d_dst, d_scr, ops); }
    int finish(const GroupPlan& P, double* d_dst, double* d_scr) { return finishing(d_means, P.means, d_dst, d_scr); }
};
template <class Op, auto Bulk, auto Fill, class Finish>
static int grouped_fold_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t live, const uint16_t* labels,
                              const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                              float* kernel_ms, Finish finishing) {
    GroupedCall<Bulk, Fill, Finish> call{{r, cubes, nq, ops}, n_groups, finishing};
    const int rc = call.labels.alloc(cubes, nq, labels, label_offset);
    if (rc != DCDF_OK) return rc;
    return cell_fold_batch<Op>(call, live, n_groups, out, out_mem, out_offset, stats, kernel_ms, call.labels.dev(), n_groups);
}
// reduce_time's statistics per cell and group of a per-instant label array (k2r_group.h): the identities by k_group_fill, MEAN
// by k_reduce_mean
extern "C" int dcdf_raster_reduce_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint16_t* labels,
                                                    const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem,
                                                    const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const bool own = ops != 0 && ops <= (RA_ALL | ROP_MEAN) && n_groups >= 1 && n_groups <= 65535 && (nq == 0 || (labels && label_offset));
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return grouped_fold_batch<GroupCell, launch_bulk_group, k_group_fill>(
        r, cubes, nq, ops, reduce_live(ops), labels, label_offset, n_groups, out, out_mem, out_offset, stats, kernel_ms,
        [ops](const DevBuf& d_means, const std::vector<MeanPiece>& means, double* d_dst, double* d_scr) {
            return ops & ROP_MEAN ? launch_over_means<k_reduce_mean>(d_means, means, d_dst, d_scr, ops) : (int)DCDF_OK;
        });
}
// Per-cell count, mean, variance and standard deviation over time (k2r_moment.h), per group of a per-instant label array or --
// labels == nullptr: the ungrouped call -- as one group every instant belongs to.  The four state arrays by k_moment_fill, MEAN /
// VAR / STD by k_moment_finish; ddof goes there only.
static int moments_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof, const uint16_t* labels,
                         const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                         float* kernel_ms) {
    return grouped_fold_batch<MomentCell, launch_bulk_moment, k_moment_fill>(
        r, cubes, nq, ops, MS_ALL, labels, label_offset, n_groups, out, out_mem, out_offset, stats, kernel_ms,
        [ops, ddof](const DevBuf& d_means, const std::vector<MeanPiece>& means, double* d_dst, double* d_scr) {
            return launch_over_means<k_moment_finish>(d_means, means, d_dst, d_scr, ops, ddof);
        });
}
extern "C" int dcdf_raster_moments_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof, double* out, int out_mem,
                                              const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const bool own = ops != 0 && ops <= MO_ALL && ddof <= 1;
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return moments_batch(r, cubes, nq, ops, ddof, nullptr, nullptr, 1, out, out_mem, out_offset, stats, kernel_ms);
}
extern "C" int dcdf_raster_moments_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof,
                                                     const uint16_t* labels, const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem,
                                                     const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const bool own = ops != 0 && ops <= MO_ALL && ddof <= 1 && n_groups >= 1 && n_groups <= 65535 && (nq == 0 || (labels && label_offset));
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return moments_batch(r, cubes, nq, ops, ddof, labels, label_offset, n_groups, out, out_mem, out_offset, stats, kernel_ms);
}
// the moments' step and finish on the host (no HIP call): continues state = (c, K, s1, s2) over x and finishes into out
extern "C" int dcdf_moments_host(const double* x, size_t n, uint32_t ddof, double state[4], double out[4]) {
    if (!state || (!x && n > 0) || ddof > 1) return DCDF_ERR_BAD_ARG;
    MomentState s{state[0], state[1], state[2], state[3]};
    for (size_t i = 0; i < n; i++) moment_step(s, x[i]);
    state[0] = s.c;
    state[1] = s.K;
    state[2] = s.s1;
    state[3] = s.s2;
    if (out) {
        double o[4];
        moment_finish(s, ddof, o);
        for (int i = 0; i < 4; i++) out[i] = o[i];
    }
    return DCDF_OK;
}
// the regression's step and finish on the host (k2r_regress.h; no HIP call): continues state = (c, K, sy, syy, se, see, sey) over the
// pairs (x[i], e[i]) and finishes into out; a value of e that is not finite is refused before the state is touched
extern "C" int dcdf_regress_host(const double* x, const double* e, size_t n, double state[7], double out[4]) {
    if (!state || ((!x || !e) && n > 0)) return DCDF_ERR_BAD_ARG;
    for (size_t i = 0; i < n; i++)
        if (!regress_finite(e[i])) return DCDF_ERR_BAD_ARG;
    RegressState s{state[0], state[1], state[2], state[3], state[4], state[5], state[6]};
    for (size_t i = 0; i < n; i++) regress_step(s, x[i], e[i]);
    const double st[7] = {s.c, s.K, s.sy, s.syy, s.se, s.see, s.sey};
    for (int i = 0; i < 7; i++) state[i] = st[i];
    if (out) {
        double o[4];
        regress_finish(s, o);
        for (int i = 0; i < 4; i++) out[i] = o[i];
    }
    return DCDF_OK;
}
// per cell, the hits of a value range over time and their runs (k2r_spell.h); cur, and LONGEST kept for LONGEST_START alone, are
// the scratch planes
struct SpellsCall : CellFoldCall<SpellPlan, uint32_t> {
    const double *lower, *upper;
    int make_plan(SpellPlan& P, const uint64_t* base, const uint64_t* sbase) { return plan_spells(r->plan(), cubes, lower, upper, nq, base, sbase, r->all_node, P); }
    int bulk(const DevBuf& units, const SegRange& g, uint32_t* d_dst, uint32_t* d_scr) {
        return launch_bulk_spell(r->d_refs.as<ChunkRef>(), units.as<SpellUnit>() + g.unit0, (uint32_t)(g.unit1 - g.unit0), d_dst, d_scr, ops);
    }
};
extern "C" int dcdf_raster_spells_batch(const dcdf_raster* r, const dcdf_cube* cubes, const double* lower, const double* upper, size_t nq,
                                        uint32_t ops, uint32_t* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    bool own = ops != 0 && ops <= SP_ALL && (nq == 0 || (lower && upper));
    for (size_t q = 0; own && q < nq && q <= 0x7fffffffu; q++) own = lower[q] == lower[q] && upper[q] == upper[q];  // a NaN bound
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, EXACT_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    SpellsCall call{{r, cubes, nq, ops}, lower, upper};
    return cell_fold_batch<SpellCell>(call, spell_live(ops), 1, out, out_mem, out_offset, stats, kernel_ms);
}
// ---- quantiles over time: per cell, order statistics of the values decode returns (k2r_quantile.h) ----------------------------
// The plan is plan_quantile_time's (k2r_plan.h): the cubes in columns, the columns in bands of a bounded slab.  A band: its
// sub-cubes decoded as stored integers (DCDF_I64: store_typed leaves n as it is) by the three launches of decode -- elided fills,
// the bulk kernel's units, the window walk's items --, then k_quantile_select (k2r_quantile.hip) over its columns.  The bands
// run one after the other on the null stream over one pooled slab.
extern "C" int dcdf_raster_quantile_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const double* probs, uint32_t n_probs,
                                               int32_t method, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                                               float* kernel_ms) {
    int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, quantile_args_ok(probs, n_probs, method), ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    const PlaneLayout L(cubes, nq, n_probs, 0);
    WindowOut W(L.planes.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    QuantilePlan P;
    rc = plan_quantile_time(r->plan(), cubes, nq, W.base.data(), quantile_slab_bytes(), r->all_node, bulk_wanted_units(), P);
    if (rc != DCDF_OK) return rc;
    DevBuf d_cols, d_segs, d_slab;
    RegionRun R;  // (units: the bulk units, cfolds: the elided fills, walk.items: the walk's items)
    rc = R.begin(W, stats, P.stats);
    if (rc != DCDF_OK || R.nothing) return rc;
    double* const d_dst = (double*)W.dst();
    K2R_HIP(d_slab.alloc_pooled(P.slab_max * sizeof(int64_t)));
    K2R_HIP(upload(d_cols, P.cols));
    K2R_HIP(upload(d_segs, P.segs));
    rc = upload_some(R.units, P.units);
    if (rc == DCDF_OK) rc = upload_some(R.cfolds, P.consts);
    if (rc == DCDF_OK) rc = upload_some(R.walk.items, P.items);
    if (rc == DCDF_OK) rc = R.start();
    if (rc != DCDF_OK) return rc;
    QuantileProbs pr{};
    for (uint32_t i = 0; i < n_probs; i++) pr.p[i] = probs[i];
    for (const QuantileBand& b : P.bands) {
        rc = launch_raster_fill_const(r, R.cfolds.as<ConstPiece>() + b.const0, (uint32_t)(b.const1 - b.const0), d_slab.p, DCDF_I64);
        if (rc == DCDF_OK)
            rc = launch_bulk_decode(r->d_refs.as<ChunkRef>(), R.units.as<BulkUnit>() + b.unit0, (uint32_t)(b.unit1 - b.unit0), d_slab.p, DCDF_I64);
        if (rc == DCDF_OK && b.item1 > b.item0)
            rc = launch_window_items_dev(r->d_refs, R.walk.items.as<WinItem>() + b.item0, (uint32_t)(b.item1 - b.item0), d_slab.p, DCDF_I64, nullptr,
                                         nullptr, r->all_node, r->all_narrow);
        if (rc == DCDF_OK)
            rc = launch_quantile_select(d_cols.as<QuantileCol>() + b.col0, (uint32_t)(b.col1 - b.col0), b.max_cells, d_segs.as<QuantileSeg>(),
                                        d_slab.as<int64_t>(), pr, n_probs, method, d_dst);
        if (rc != DCDF_OK) return rc;
    }
    return R.end(W, true, kernel_ms);
}
// ---- regression over time: per cell, the least-squares line of its series against a per-instant regressor (k2r_regress.h) -------
// The plan is plan_regress_time's (k2r_plan.h): the quantiles' bands over the same slab and cap, and per cube the ordered
// records and the CSR of its groups.  A band: the three launches of decode as above, then k_regress_stream (k2r_regress.hip)
// over its columns, which reads the slab once and writes every element of the planes.  labels == nullptr: the ungrouped call.
static int regress_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const double* regressor,
                         const uint64_t* regressor_offset, const uint16_t* labels, const uint64_t* label_offset, uint32_t n_groups, double* out,
                         int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const PlaneLayout L(cubes, nq, popc32(ops) * n_groups, 0);
    WindowOut W(L.planes.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    RegressPlan P;
    int rc = plan_regress_time(r->plan(), cubes, nq, W.base.data(), quantile_slab_bytes(), r->all_node, bulk_wanted_units(), regressor,
                               regressor_offset, labels, label_offset, n_groups, P);
    if (rc != DCDF_OK) return rc;
    DevBuf d_cols, d_segs, d_recs, d_start, d_slab;
    RegionRun R;  // (units: the bulk units, cfolds: the elided fills, walk.items: the walk's items)
    rc = R.begin(W, stats, P.q.stats);
    if (rc != DCDF_OK || R.nothing) return rc;
    double* const d_dst = (double*)W.dst();
    K2R_HIP(d_slab.alloc_pooled(P.q.slab_max * sizeof(int64_t)));
    K2R_HIP(upload(d_cols, P.cols));
    K2R_HIP(upload(d_segs, P.q.segs));
    K2R_HIP(upload(d_start, P.start));
    rc = upload_some(d_recs, P.recs);  // (none when no instant is in a group)
    if (rc == DCDF_OK) rc = upload_some(R.units, P.q.units);
    if (rc == DCDF_OK) rc = upload_some(R.cfolds, P.q.consts);
    if (rc == DCDF_OK) rc = upload_some(R.walk.items, P.q.items);
    if (rc == DCDF_OK) rc = R.start();
    if (rc != DCDF_OK) return rc;
    for (const QuantileBand& b : P.q.bands) {
        rc = launch_raster_fill_const(r, R.cfolds.as<ConstPiece>() + b.const0, (uint32_t)(b.const1 - b.const0), d_slab.p, DCDF_I64);
        if (rc == DCDF_OK)
            rc = launch_bulk_decode(r->d_refs.as<ChunkRef>(), R.units.as<BulkUnit>() + b.unit0, (uint32_t)(b.unit1 - b.unit0), d_slab.p, DCDF_I64);
        if (rc == DCDF_OK && b.item1 > b.item0)
            rc = launch_window_items_dev(r->d_refs, R.walk.items.as<WinItem>() + b.item0, (uint32_t)(b.item1 - b.item0), d_slab.p, DCDF_I64, nullptr,
                                         nullptr, r->all_node, r->all_narrow);
        if (rc == DCDF_OK)
            rc = launch_regress_stream(d_cols.as<RegressCol>() + b.col0, (uint32_t)(b.col1 - b.col0), b.max_cells, d_segs.as<QuantileSeg>(),
                                       d_recs.as<RegressRec>(), d_start.as<uint32_t>(), n_groups, d_slab.as<int64_t>(), ops, d_dst);
        if (rc != DCDF_OK) return rc;
    }
    return R.end(W, true, kernel_ms);
}
extern "C" int dcdf_raster_regress_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const double* regressor,
                                              const uint64_t* regressor_offset, double* out, int out_mem, const uint64_t* out_offset,
                                              uint64_t stats[3], float* kernel_ms) {
    const bool own = ops != 0 && ops <= RO_ALL && !regressor == !regressor_offset;
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return regress_batch(r, cubes, nq, ops, regressor, regressor_offset, nullptr, nullptr, 1, out, out_mem, out_offset, stats, kernel_ms);
}
extern "C" int dcdf_raster_regress_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const double* regressor,
                                                     const uint64_t* regressor_offset, const uint16_t* labels, const uint64_t* label_offset,
                                                     uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                                                     float* kernel_ms) {
    const bool own = ops != 0 && ops <= RO_ALL && !regressor == !regressor_offset && n_groups >= 1 && n_groups <= 65535 &&
                     (nq == 0 || (labels && label_offset));
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return regress_batch(r, cubes, nq, ops, regressor, regressor_offset, labels, label_offset, n_groups, out, out_mem, out_offset, stats, kernel_ms);
}
// ---- rolling windows over time: per cell, the extremes of the sums or means of every w consecutive instants (k2r_rolling.h) -------
// The plan is plan_rolling_time's (k2r_plan.h): the quantiles' bands over the same slab and cap, and per cube its instant table,
// the ordered ends of its groups' windows and their CSR.  A band: the three launches of decode as above, then k_rolling_stream
// (k2r_rolling.hip) over its columns, which writes every element of the planes.  labels == nullptr: the plain call.
static int rolling_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window, uint32_t min_count, int32_t kind,
                         const uint16_t* labels, const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem,
                         const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const PlaneLayout L(cubes, nq, popc32(ops) * n_groups, 0);
    WindowOut W(L.planes.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    RollingPlan P;
    int rc = plan_rolling_time(r->plan(), cubes, nq, W.base.data(), quantile_slab_bytes(), r->all_node, bulk_wanted_units(), ops, window,
                               min_count, kind, labels, label_offset, n_groups, P);
    if (rc != DCDF_OK) return rc;
    DevBuf d_cols, d_segs, d_ends, d_start, d_seg_of, d_slab;
    RegionRun R;  // (units: the bulk units, cfolds: the elided fills, walk.items: the walk's items)
    rc = R.begin(W, stats, P.q.stats);
    if (rc != DCDF_OK || R.nothing) return rc;
    double* const d_dst = (double*)W.dst();
    K2R_HIP(d_slab.alloc_pooled(P.q.slab_max * sizeof(int64_t)));
    K2R_HIP(upload(d_cols, P.cols));
    K2R_HIP(upload(d_segs, P.q.segs));
    K2R_HIP(upload(d_start, P.start));
    K2R_HIP(upload(d_seg_of, P.seg_of));
    rc = upload_some(d_ends, P.ends);  // (none when no window ends in a group)
    if (rc == DCDF_OK) rc = upload_some(R.units, P.q.units);
    if (rc == DCDF_OK) rc = upload_some(R.cfolds, P.q.consts);
    if (rc == DCDF_OK) rc = upload_some(R.walk.items, P.q.items);
    if (rc == DCDF_OK) rc = R.start();
    if (rc != DCDF_OK) return rc;
    for (const QuantileBand& b : P.q.bands) {
        rc = launch_raster_fill_const(r, R.cfolds.as<ConstPiece>() + b.const0, (uint32_t)(b.const1 - b.const0), d_slab.p, DCDF_I64);
        if (rc == DCDF_OK)
            rc = launch_bulk_decode(r->d_refs.as<ChunkRef>(), R.units.as<BulkUnit>() + b.unit0, (uint32_t)(b.unit1 - b.unit0), d_slab.p, DCDF_I64);
        if (rc == DCDF_OK && b.item1 > b.item0)
            rc = launch_window_items_dev(r->d_refs, R.walk.items.as<WinItem>() + b.item0, (uint32_t)(b.item1 - b.item0), d_slab.p, DCDF_I64, nullptr,
                                         nullptr, r->all_node, r->all_narrow);
        if (rc == DCDF_OK)
            rc = launch_rolling_stream(d_cols.as<RollingCol>() + b.col0, (uint32_t)(b.col1 - b.col0), b.max_cells, d_segs.as<QuantileSeg>(),
                                       d_ends.as<uint32_t>(), d_start.as<uint32_t>(), d_seg_of.as<uint32_t>(), n_groups, d_slab.as<int64_t>(), ops,
                                       window, min_count, kind, d_dst);
        if (rc != DCDF_OK) return rc;
    }
    return R.end(W, true, kernel_ms);
}
extern "C" int dcdf_raster_rolling_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window,
                                              uint32_t min_count, int32_t kind, double* out, int out_mem, const uint64_t* out_offset,
                                              uint64_t stats[3], float* kernel_ms) {
    const bool own = rolling_args_ok(ops, window, min_count, kind);
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return rolling_batch(r, cubes, nq, ops, window, min_count, kind, nullptr, nullptr, 1, out, out_mem, out_offset, stats, kernel_ms);
}
extern "C" int dcdf_raster_rolling_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window,
                                                     uint32_t min_count, int32_t kind, const uint16_t* labels, const uint64_t* label_offset,
                                                     uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                                                     float* kernel_ms) {
    const bool own = rolling_args_ok(ops, window, min_count, kind) && n_groups >= 1 && n_groups <= 65535 && (nq == 0 || (labels && label_offset));
    const int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, ANY_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    return rolling_batch(r, cubes, nq, ops, window, min_count, kind, labels, label_offset, n_groups, out, out_mem, out_offset, stats, kernel_ms);
}
// ---- reduce over space: per-instant min / max / sum / count / mean of the selected cells of a cube (k2r_space.h) ------------
// The plan is plan_reduce_space's (k2r_plan.h): records of the pieces in a pooled scratch array, in blocks [slot][instant] that
// k_space_finish folds into the cubes' series.  Instants are independent: one launch of each kind takes the work of a whole batch.
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
extern "C" int dcdf_raster_reduce_space_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint8_t* mask,
                                              const uint64_t* mask_offset, int mask_mem, double* out, int out_mem, const uint64_t* out_offset,
                                              uint64_t stats[3], float* kernel_ms) {
    int rc = region_begin(r, cubes, nq, out, out_offset, out_mem,
                          ops != 0 && ops <= (RA_ALL | ROP_MEAN) && CubeMasks::args_ok(mask, mask_offset, mask_mem), EXACT_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    const uint32_t live = reduce_live(ops), n_out = popc32(ops);
    // where the series go: cube q's are n_out "instants" of one row of [instants] to WindowOut
    std::vector<dcdf_cube> series(nq, dcdf_cube{});
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end != c.start) series[q] = dcdf_cube{0, n_out, 0, 1, 0, c.end - c.start};
    }
    WindowOut W(series.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    CubeMasks M(cubes, nq, mask, mask_offset, mask_mem);
    SpacePlan P(reduce_slab_cells());
    rc = plan_reduce_space(r->plan(), cubes, nq, W.base.data(), M.moff.data(), r->all_node, space_record_cap(), bulk_wanted_units(), P);
    if (rc != DCDF_OK) return rc;
    DevBuf d_jobs, d_recs;
    RegionRun R;
    rc = R.begin(W, stats, P.stats);
    if (rc != DCDF_OK || R.nothing) return rc;
    double* const d_dst = (double*)W.dst();
    rc = M.stage(cubes, nq, mask_offset);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(d_recs.alloc_pooled(P.rec_max * sizeof(SpacePartial)));
    rc = R.upload(P);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(upload(d_jobs, P.jobs));
    rc = R.start();
    if (rc != DCDF_OK) return rc;
    SpacePartial* const recs = d_recs.as<SpacePartial>();
    for (const SpaceBatch& b : P.batches) {
        rc = R.fold_consts<k_space_fold, SpaceFold>(r, b, 1, M.p, recs);
        if (rc == DCDF_OK)
            rc = launch_bulk_space(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), R.units.as<SpaceUnit>() + b.unit0, (uint32_t)(b.unit1 - b.unit0), M.p,
                                   recs, live);
        if (rc == DCDF_OK) rc = R.walk.run<k_space_fold>(r, P.walk, b, std::min<uint32_t>(P.walk.fold_nt, 1024), M.p, recs);
        if (rc != DCDF_OK) return rc;
        hipLaunchKernelGGL(k_space_finish, dim3((uint32_t)std::min<size_t>(b.job1 - b.job0, 1u << 20), std::min<uint32_t>(b.job_nt, 1024)), dim3(256), 0,
                           0, d_jobs.as<SpaceJob>() + b.job0, (uint32_t)(b.job1 - b.job0), recs, d_dst, ops);
        K2R_HIP(hipGetLastError());
    }
    return R.end(W, true, kernel_ms);
}
// ---- value histograms: per instant, how many selected cells of a cube fall into every bin of shared edges (k2r_hist.h) -------
// The plan is plan_histogram's (k2r_plan.h).  Every piece adds its counts to the cube's own [instants][bins] array with device-scope
// 64-bit atomic adds; the call zeroes exactly those arrays first.  Integer adds commute: the result depends on no order.
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
    int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, hist_edges_ok(edges, n_bins) && CubeMasks::args_ok(mask, mask_offset, mask_mem),
                          EXACT_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    // where the counts go: cube q's are "instants" of one row of [bins] to WindowOut
    std::vector<dcdf_cube> rows(nq, dcdf_cube{});
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end != c.start) rows[q] = dcdf_cube{0, c.end - c.start, 0, 1, 0, n_bins};
    }
    WindowOut W(rows.data(), nq, out, out_offset, sizeof(uint64_t), out_mem == DCDF_MEM_DEVICE);
    CubeMasks M(cubes, nq, mask, mask_offset, mask_mem);
    HistPlan P(reduce_slab_cells());
    rc = plan_histogram(r->plan(), cubes, nq, W.base.data(), M.moff.data(), edges, n_bins, r->all_node, bulk_wanted_units(), P);
    if (rc != DCDF_OK) return rc;
    put_stats(stats, P.stats);
    if (W.total == 0) return DCDF_OK;
    DevBuf d_units, d_cfolds, d_thr, d_edges;
    WalkDev D;
    if (!W.to_dev) K2R_HIP(W.stage.alloc_pooled(W.total * W.es));
    uint64_t* const d_dst = (uint64_t*)W.dst();
    rc = M.stage(cubes, nq, mask_offset);
    if (rc != DCDF_OK) return rc;
    if (!P.units.empty()) {
        K2R_HIP(upload(d_units, P.units));
        K2R_HIP(upload(d_thr, P.thr));
    }
    rc = upload_some(d_cfolds, P.cfolds);
    if (rc == DCDF_OK) rc = D.upload(P.walk);
    if (rc != DCDF_OK) return rc;
    if (!P.cfolds.empty() || !P.walk.folds.empty()) K2R_HIP(upload(d_edges, std::vector<double>(edges, edges + n_bins + 1)));
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
    if (!P.cfolds.empty()) {
        hipLaunchKernelGGL(k_hist_fold, dim3((uint32_t)std::min<size_t>(P.cfolds.size(), 1u << 20), 1), dim3(256), 0, 0, d_cfolds.as<HistFold>(),
                           (uint32_t)P.cfolds.size(), nullptr, r->d_vals.as<int64_t>(), M.p, d_edges.as<double>(), n_bins, d_dst);
        K2R_HIP(hipGetLastError());
    }
    rc = launch_bulk_hist(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), d_units.as<HistUnit>(), (uint32_t)P.units.size(), M.p, d_thr.as<int32_t>(),
                          n_bins, d_dst);
    for (size_t s = 0; rc == DCDF_OK && s < P.walk.slabs.size(); s++) {
        const Slab& sl = P.walk.slabs[s];
        rc = launch_window_items_dev(r->d_refs, D.items.as<WinItem>() + sl.item0, (uint32_t)(sl.item1 - sl.item0), D.slab.p, DCDF_I64, nullptr, nullptr,
                                     r->all_node, r->all_narrow);
        if (rc != DCDF_OK) break;
        hipLaunchKernelGGL(k_hist_fold, dim3((uint32_t)std::min<size_t>(sl.fold1 - sl.fold0, 1u << 20), std::min<uint32_t>(P.walk.fold_nt, 1024)),
                           dim3(256), 0, 0, D.folds.as<HistFold>() + sl.fold0, (uint32_t)(sl.fold1 - sl.fold0), D.slab.as<int64_t>(), nullptr, M.p,
                           d_edges.as<double>(), n_bins, d_dst);
        K2R_HIP(hipGetLastError());
    }
    if (rc != DCDF_OK) return rc;
    return batch_epilogue(W, ev, true, kernel_ms);
}
// ---- zonal statistics: per (zone, instant) of a cube, reduce_space's statistics over the cells that carry the zone's label ----
// The plan is plan_zonal's (k2r_plan.h), the accumulators and their arithmetic k2r_zonal.h's.  A batch of the plan: its entries
// zeroed, every piece's adds (elided pieces, the bulk kernel's units, the window walk's slabs), then k_zonal_finish.
// The labels are CubeLabels.
// A thread takes a run of consecutive cells of the piece (row-major) and folds every run of equal labels among them into one
// add per (zone, instant): neighbours mostly share a zone.  A piece of the window walk's slab: a workgroup per (piece, instant),
// the cells' stored integers widened by the leaf's own encoding, two-limb sums since |m| <= 2^63.  An elided piece (blockIdx.y == 0
// alone): per run of n cells of one zone and per instant, value x n (space_mul_m).
__global__ void __launch_bounds__(256)
k_zonal_fold(const ZonalFold* __restrict__ ps, uint32_t n, const int64_t* __restrict__ slab, const int64_t* __restrict__ vals,
             const uint16_t* __restrict__ labels, uint32_t n_zones, uint64_t* acc, uint32_t live) {
    const bool ext = (live & (RA_MIN | RA_MAX)) != 0, add = (live & RA_SUM) != 0;
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const ZonalFold P = ps[p];
        const uint64_t cells = (uint64_t)P.rows * P.cols, per = (cells + blockDim.x - 1) / blockDim.x;
        const uint64_t e0 = std::min<uint64_t>(cells, threadIdx.x * per), e1 = std::min<uint64_t>(cells, e0 + per);
        const uint32_t scale = space_scale(P.enc, P.fbits);
        if (P.elided && blockIdx.y != 0) continue;
        for (uint32_t t = P.elided ? 0u : blockIdx.y; t < (P.elided ? 1u : P.nt); t += gridDim.y) {
            SpaceAcc a{0, 0, __builtin_nan(""), __builtin_nan(""), 0};
            uint32_t run = ZONAL_NONE;  // the label of the current run; a.cnt: its cells (elided) or its non-NaN values
            for (uint64_t e = e0; e <= e1; e++) {
                uint32_t l = ZONAL_NONE;
                if (e < e1) {
                    l = labels[P.m_off + e / P.cols * P.m_sr + e % P.cols];
                    if (l >= n_zones) l = ZONAL_NONE;
                }
                if (l != run) {  // (e == e1 closes the last run)
                    if (run != ZONAL_NONE && a.cnt != 0) {
                        if (!P.elided) {
                            zonal_add(acc, P.acc + (uint64_t)run * P.a_st + t, a.hi, a.lo, scale, a.cnt, a.mn, a.mx, ext, add);
                        } else {
                            for (uint32_t i = 0; i < P.nt; i++) {
                                const int64_t v = vals[P.src + i];
                                const double x = reduce_widen(P.enc, P.fbits, v);
                                if (x != x) continue;
                                uint64_t hi, lo;
                                space_mul_m(hi, lo, space_m(P.enc, v), a.cnt);
                                zonal_add(acc, P.acc + (uint64_t)run * P.a_st + i, hi, lo, scale, a.cnt, x, x, ext, add);
                            }
                        }
                    }
                    a = SpaceAcc{0, 0, __builtin_nan(""), __builtin_nan(""), 0};
                    run = l;
                }
                if (l == ZONAL_NONE) continue;
                if (P.elided) {
                    a.cnt += 1u;
                    continue;
                }
                const int64_t v = slab[P.src + (uint64_t)t * cells + e];
                const double x = reduce_widen(P.enc, P.fbits, v);
                if (x == x) {
                    space_add_m(a.hi, a.lo, space_m(P.enc, v));
                    a.cnt += 1u;
                    a.mn = fmin(a.mn, x);
                    a.mx = fmax(a.mx, x);
                }
            }
        }
    }
}
// A thread per (zone, instant) of a span: the limbs into one 192-bit integer and one rounding, the keys back into doubles, one
// division for the mean; the span's part of the cube's matrices by plain stores.
__global__ void __launch_bounds__(256)
k_zonal_finish(const ZonalSpan* __restrict__ spans, uint32_t n, uint32_t n_zones, const uint64_t* __restrict__ acc, double* dst, uint32_t ops) {
    for (uint32_t s = blockIdx.x; s < n; s += gridDim.x) {
        const ZonalSpan S = spans[s];
        const uint64_t entries = (uint64_t)n_zones * S.nt;
        for (uint64_t e = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; e < entries; e += (uint64_t)gridDim.y * blockDim.x) {
            const __attribute__((address_space(1))) uint64_t* const A = (const __attribute__((address_space(1))) uint64_t*)acc + (S.acc + e) * ZONAL_WORDS;
            const uint64_t cnt = A[ZA_CNT], kmin = A[ZA_MIN], kmax = A[ZA_MAX];
            int64_t limbs[6];
#pragma unroll
            for (uint32_t i = 0; i < 6u; i++) limbs[i] = (int64_t)A[ZA_LIMB + i];
            U192 v;
            zonal_fold(limbs, v);
            const double sum = space_round(v);
            __attribute__((address_space(1))) double* o = (__attribute__((address_space(1))) double*)dst + (S.o_off + e / S.nt * S.o_zone + e % S.nt);
            if (ops & RA_MIN) { *o = kmin ? zonal_unkey(~kmin) : __builtin_nan(""); o += S.o_stat; }
            if (ops & RA_MAX) { *o = kmax ? zonal_unkey(kmax) : __builtin_nan(""); o += S.o_stat; }
            if (ops & RA_SUM) { *o = sum; o += S.o_stat; }
            if (ops & RA_COUNT) { *o = (double)cnt; o += S.o_stat; }
            if (ops & ROP_MEAN) *o = cnt == 0 ? __builtin_nan("") : sum / (double)cnt;
        }
    }
}
extern "C" int dcdf_zonal_fold_limbs(const int64_t limbs[6], double* sum) {
    if (!limbs || !sum) return DCDF_ERR_BAD_ARG;
    const int64_t l[6] = {limbs[0], limbs[1], limbs[2], limbs[3], limbs[4], limbs[5]};
    U192 v;
    if (!zonal_fold(l, v)) return DCDF_ERR_BAD_ARG;
    *sum = space_round(v);
    return DCDF_OK;
}
extern "C" int dcdf_raster_zonal_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint16_t* labels,
                                       const uint64_t* label_offset, int label_mem, uint32_t n_zones, double* out, int out_mem,
                                       const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms) {
    const bool own = ops != 0 && ops <= (RA_ALL | ROP_MEAN) && n_zones >= 1 && n_zones <= 65535u && (nq == 0 || (labels && label_offset)) &&
                     (label_mem == DCDF_MEM_HOST || label_mem == DCDF_MEM_DEVICE);
    int rc = region_begin(r, cubes, nq, out, out_offset, out_mem, own, EXACT_FLOATS, stats, kernel_ms);
    if (rc != DCDF_OK || nq == 0) return rc;
    const uint32_t live = reduce_live(ops), n_out = popc32(ops);
    // where the matrices go: cube q's are n_out "instants" of [zones][instants] to WindowOut
    std::vector<dcdf_cube> mats(nq, dcdf_cube{});
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end != c.start) mats[q] = dcdf_cube{0, n_out, 0, n_zones, 0, c.end - c.start};
    }
    WindowOut W(mats.data(), nq, out, out_offset, sizeof(double), out_mem == DCDF_MEM_DEVICE);
    CubeLabels M(cubes, nq, labels, label_offset, label_mem);
    ZonalPlan P(reduce_slab_cells());
    rc = plan_zonal(r->plan(), cubes, nq, W.base.data(), M.moff.data(), n_zones, r->all_node, zonal_acc_cap(), bulk_wanted_units(), P);
    if (rc != DCDF_OK) return rc;
    DevBuf d_spans, d_acc;
    RegionRun R;
    rc = R.begin(W, stats, P.stats);
    if (rc != DCDF_OK || R.nothing) return rc;
    double* const d_dst = (double*)W.dst();
    rc = M.stage(cubes, nq, label_offset);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(d_acc.alloc_pooled(P.entries_max * ZONAL_BYTES));
    rc = R.upload(P);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(upload(d_spans, P.spans));
    rc = R.start();
    if (rc != DCDF_OK) return rc;
    uint64_t* const acc = d_acc.as<uint64_t>();
    for (const ZonalBatch& b : P.batches) {
        K2R_HIP(hipMemsetAsync(acc, 0, b.entries * ZONAL_BYTES, 0));
        rc = R.fold_consts<k_zonal_fold, ZonalFold>(r, b, 1, M.p, n_zones, acc, live);
        if (rc == DCDF_OK)
            rc = launch_bulk_zonal(r->d_refs.as<ChunkRef>(), r->d_enc.as<uint8_t>(), R.units.as<ZonalUnit>() + b.unit0, (uint32_t)(b.unit1 - b.unit0), M.p,
                                   n_zones, acc, live);
        if (rc == DCDF_OK) rc = R.walk.run<k_zonal_fold>(r, P.walk, b, std::min<uint32_t>(P.walk.fold_nt, 1024), M.p, n_zones, acc, live);
        if (rc != DCDF_OK) return rc;
        const uint64_t big = (uint64_t)n_zones * P.span_nt;
        hipLaunchKernelGGL(k_zonal_finish, dim3((uint32_t)std::min<size_t>(b.span1 - b.span0, 1u << 16), (uint32_t)std::min<uint64_t>((big + 255) / 256, 4096)),
                           dim3(256), 0, 0, d_spans.as<ZonalSpan>() + b.span0, (uint32_t)(b.span1 - b.span0), n_zones, acc, d_dst, ops);
        K2R_HIP(hipGetLastError());
    }
    return R.end(W, true, kernel_ms);
}
