// k2r_plan.h -- how the region calls of a raster (decode, reduce_time, reduce_time_groups, reduce_space, histogram, spells, zonal, quantile_time, regress_time, rolling_time:
// k2r_raster_region.hip)
// turn a batch of cubes into device work.  Host code only, no HIP header: tests/sim/plan_check.cpp runs it on a CPU.
//
// A cube is cut into pieces, one per leaf it meets (raster_pieces).  A piece is of one of three kinds: on an elided leaf (one
// value per instant: dcdf_raster::d_vals), on a chunk the bulk kernels take (side-16 table, 32-bit values) -- it becomes one unit
// per 64 x 64 region of the chunk's own grid --, or on any other chunk -- the window walk decodes it, for the reductions into a
// slab of stored integers a fold kernel then reads.  The planner sees the raster's geometry and a table of its leaves, never a
// chunk.  Everything that reaches a launch keeps one order: cubes in batch order, then segment, tile row, tile column, then the
// regions' rows, columns, then instants.
#pragma once
#include <map>
#include <utility>

#include "k2r_bulk.h"
#include "k2r_group.h"
#include "k2r_hist.h"
#include "k2r_items.h"
#include "k2r_quantile.h"
#include "k2r_reduce.h"
#include "k2r_regress.h"
#include "k2r_rolling.h"
#include "k2r_space.h"
#include "k2r_spell.h"
#include "k2r_zonal.h"

// an elided piece of a decode: one value per instant over a rectangle of the window (k_raster_fill_const; outside the namespace,
// where the kernels' mangled names have it)
struct ConstPiece {
    uint32_t leaf, ls, le, rows, cols, out_sr;  // leaf-local instants [ls, le), the rectangle, the window's row stride
    uint64_t out_off, out_st;                   // element of (ls, top, left) in `out`; the window's instant stride
};

namespace k2r {

// The per-piece path -- raster_pieces, plan_pieces, plan_units and the callers' lambdas -- is forced inline: left to itself the
// compiler keeps them out of line and builds every Piece in memory, which a batch of many small cubes pays for per piece.
#define K2R_PLAN_INLINE inline __attribute__((always_inline))
#define K2R_PLAN_LAMBDA __attribute__((always_inline))

// ---- what the planner sees of a raster ---------------------------------------------------------------------------------------
struct PlanLeaf {
    uint32_t row0, col0;  // where the leaf starts inside its chunk
    int32_t enc;          // what the folds widen with: the leaf's own for an elided leaf, else the chunk's
    uint32_t fbits;
    uint8_t elided, bulk_ok;  // bulk_ok: the chunk has a side-16 table and 32-bit values
};
struct PlanRaster {
    uint32_t T, R, C, tile, cs, nti, ntj;
    const PlanLeaf* leaves;  // [(segment * nti + ti) * ntj + tj]
};
inline int plan_bounds(const PlanRaster& g, const dcdf_cube* cubes, size_t nq) {
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end > g.T || c.bottom > g.R || c.right > g.C) return DCDF_ERR_BOUNDS;
    }
    return DCDF_OK;
}

// room to start a list with: a batch of nq cubes has at least nq pieces (many small cubes: no growth by doubling on the way there)
inline size_t plan_reserve(size_t nq) { return std::min<size_t>(nq, (size_t)1 << 20); }

// ---- pieces ------------------------------------------------------------------------------------------------------------------
// the pieces of one dataset-level cube (normalised, not empty): f(leaf id, leaf-local cube, raster origin of the leaf)
template <class F>
K2R_PLAN_INLINE void raster_pieces(const PlanRaster& g, const dcdf_cube& c, F&& f) {
    for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++)
        for (uint32_t ti = c.top / g.tile; ti <= (c.bottom - 1) / g.tile; ti++)
            for (uint32_t tj = c.left / g.tile; tj <= (c.right - 1) / g.tile; tj++) {
                const uint32_t t0 = seg * g.cs, r0 = ti * g.tile, c0 = tj * g.tile;
                const dcdf_cube l{std::max(c.start, t0) - t0, std::min(c.end, t0 + g.cs) - t0, std::max(c.top, r0) - r0,
                                  std::min(c.bottom, r0 + g.tile) - r0, std::max(c.left, c0) - c0, std::min(c.right, c0 + g.tile) - c0};
                f((uint32_t)(((uint64_t)seg * g.nti + ti) * g.ntj + tj), l, t0, r0, c0);
            }
}
enum PieceKind : uint32_t { PIECE_BULK = 0, PIECE_WALK = 1, PIECE_CONST = 2 };  // (the order of the calls' stats[3])
struct Piece {
    uint32_t leaf;
    PieceKind kind;
    dcdf_cube l, k;       // the piece in the leaf's coordinates and in its chunk's (l moved by row0 / col0)
    uint32_t t0, r0, c0;  // the leaf's origin in the raster
    int32_t enc;          // PlanLeaf's
    uint32_t fbits;
    uint32_t dt;          // the piece's first instant, counted from the cube's
    uint64_t in_win;      // its first cell in the cube's [rows][cols] plane
    uint64_t cells;
    uint32_t nt() const { return l.end - l.start; }
    uint32_t rows() const { return l.bottom - l.top; }
    uint32_t cols() const { return l.right - l.left; }
};
// every piece of cube c, classified; its cells are added to stats[kind]
template <class F>
K2R_PLAN_INLINE void plan_pieces(const PlanRaster& g, const dcdf_cube& c, uint64_t stats[3], F&& f) {
    raster_pieces(g, c, [&](uint32_t leaf, const dcdf_cube& l, uint32_t t0, uint32_t r0, uint32_t c0) K2R_PLAN_LAMBDA {
        const PlanLeaf& L = g.leaves[leaf];
        Piece p{leaf, L.elided ? PIECE_CONST : L.bulk_ok ? PIECE_BULK : PIECE_WALK, l,
                dcdf_cube{l.start, l.end, L.row0 + l.top, L.row0 + l.bottom, L.col0 + l.left, L.col0 + l.right}, t0, r0, c0, L.enc, L.fbits,
                t0 + l.start - c.start, (uint64_t)(r0 + l.top - c.top) * (c.right - c.left) + (c0 + l.left - c.left), cube_cells(l)};
        stats[p.kind] += p.cells;
        f(p);
    });
}
// One unit per 64 x 64 region of the chunk's grid that a bulk piece meets: the fields every unit type starts with (BulkUnit's
// first 24 bytes) are set here, own(u) sets the rest.
template <class U, class F>
K2R_PLAN_INLINE void plan_units(const Piece& p, std::vector<U>& units, F&& own) {
    const dcdf_cube& k = p.k;
    for (uint32_t rr = k.top & ~(BULK_REGION - 1); rr < k.bottom; rr += BULK_REGION)
        for (uint32_t rc = k.left & ~(BULK_REGION - 1); rc < k.right; rc += BULK_REGION) {
            U u{};
            u.chunk = p.leaf;
            u.t0 = k.start;
            u.t1 = k.end;
            u.rr = (uint16_t)rr;
            u.rc = (uint16_t)rc;
            u.top = (uint16_t)std::max(rr, k.top);
            u.bottom = (uint16_t)std::min(rr + BULK_REGION, k.bottom);
            u.left = (uint16_t)std::max(rc, k.left);
            u.right = (uint16_t)std::min(rc + BULK_REGION, k.right);
            own(u);
            units.push_back(u);
        }
}
// the place of unit u's first cell inside its piece, in a plane of row stride sr
template <class U>
inline uint64_t unit_in_piece(const U& u, const Piece& p, uint64_t sr) { return (uint64_t)(u.top - p.k.top) * sr + (u.left - p.k.left); }
// Few units: the instants of every unit of units[from ..) in several workgroups (bulk_parts; each part decodes its Snapshot
// again).  advance(v, dt) moves a part's own offset dt instants on.  wanted: bulk_wanted_units().
template <class U, class F>
inline void plan_time_split(std::vector<U>& units, size_t from, uint32_t wanted, F&& advance) {
    const size_t nu = units.size() - from;
    if (bulk_parts(nu, ~0u, wanted) <= 1) return;  // enough units, however long (the usual case: no pass over them)
    uint32_t max_nt = 0;
    for (size_t i = from; i < units.size(); i++) max_nt = std::max(max_nt, units[i].t1 - units[i].t0);
    const uint32_t parts = bulk_parts(nu, max_nt, wanted);
    if (parts <= 1) return;
    std::vector<U> split;
    split.reserve(nu * parts);
    for (size_t i = from; i < units.size(); i++) {
        const U& u = units[i];
        const uint32_t nt = u.t1 - u.t0, np = bulk_parts(nu, nt, wanted);
        for (uint32_t j = 0; j < np; j++) {
            U v = u;
            v.t0 = bulk_part(u.t0, nt, np, j);
            v.t1 = bulk_part(u.t0, nt, np, j + 1);
            advance(v, v.t0 - u.t0);
            if (v.t1 > v.t0) split.push_back(v);
        }
    }
    units.resize(from);
    units.insert(units.end(), split.begin(), split.end());
}

// ---- the window walk's pieces, in slabs --------------------------------------------------------------------------------------
// One slab: a walk launch over items[item0, item1) decodes stored integers into the slab, a fold launch over folds[fold0, fold1)
// reads them.  A slab takes whole pieces up to `cap` cells; a piece beyond that is cut in time and each part gets a slab of its
// own: two parts of one piece share their cells (reduce_time's state planes), so one fold launch must never hold both.
struct Slab {
    size_t item0, item1, fold0, fold1;
};
// the instants [a, b) of a walk piece's cube
inline dcdf_cube cube_instants(dcdf_cube k, uint32_t a, uint32_t b) {
    k.end = k.start + b;
    k.start += a;
    return k;
}
template <class Fold>
struct SlabCutter {
    uint64_t cap, used = 0, slab_max = 0;  // cells: the bound, of the current slab, of the largest
    uint32_t fold_nt = 1;                  // the longest part
    Slab cur{0, 0, 0, 0};
    std::vector<WinItem> items;
    std::vector<Fold> folds;
    std::vector<Slab> slabs;
    explicit SlabCutter(uint64_t cap_) : cap(cap_) {}
    void flush() {
        cur.item1 = items.size();
        cur.fold1 = folds.size();
        if (cur.fold1 > cur.fold0) slabs.push_back(cur);
        slab_max = std::max(slab_max, used);
        cur = Slab{items.size(), 0, folds.size(), 0};
        used = 0;
    }
    // a walk piece of nt instants of `plane` cells: part(a, b, src) pushes the fold and the items of its instants [a, b), whose
    // integers start at element src of the slab
    template <class F>
    void add(uint32_t nt, uint64_t plane, F&& part) {
        const uint32_t cut = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, cap / plane));
        if (cut < nt || used + (uint64_t)nt * plane > cap) flush();
        for (uint32_t a = 0; a < nt; a += cut) {
            const uint32_t b = std::min(nt, a + cut);
            part(a, b, used);
            fold_nt = std::max(fold_nt, b - a);
            used += (uint64_t)(b - a) * plane;
            if (cut < nt) flush();
        }
    }
    // The walk piece on leaf `chunk` over the chunk-level cube k, whose fold without the slab offset is f: every part gets f with
    // its own nt and src, and own(fold, a) moves what else depends on the part's first instant a (counted from k's).
    template <class F>
    K2R_PLAN_INLINE void add_piece(uint32_t chunk, const dcdf_cube& k, const Fold& f, bool node_wise, F&& own) {
        add(k.end - k.start, (uint64_t)f.rows * f.cols, [&](uint32_t a, uint32_t b, uint64_t src) {
            Fold w = f;
            w.nt = b - a;
            w.src = src;
            own(w, a);
            window_items(chunk, cube_instants(k, a, b), src, items, node_wise);
            folds.push_back(w);
        });
    }
};
// a walk piece kept until its slab is known: the leaf, the chunk-level cube, and its fold without the slab offset
template <class Fold>
struct WalkPiece {
    uint32_t chunk;
    dcdf_cube k;
    Fold f;
};

// ---- what every reduction plan carries ---------------------------------------------------------------------------------------
// The three lists a launch reads -- bulk units, elided folds, the walk's slabs -- and the cells of each kind.  A PlanRange is a
// stretch of all three that is launched together: mark() opens one at the lists' ends, close() ends it there.
struct PlanRange {
    size_t unit0, unit1, const0, const1, slab0, slab1;
};
template <class Unit, class Fold>
struct ReducePlan {
    std::vector<Unit> units;
    std::vector<Fold> cfolds;
    SlabCutter<Fold> walk;
    uint64_t stats[3] = {0, 0, 0};
    explicit ReducePlan(uint64_t slab_cap) : walk(slab_cap) {}
    // what a launch's 32-bit counts cannot take
    bool full() const { return units.size() > 0x3fffffffull || walk.items.size() > 0xfffffff0ull || cfolds.size() + walk.folds.size() > 0xfffffff0ull; }
    PlanRange mark() const { return PlanRange{units.size(), 0, cfolds.size(), 0, walk.slabs.size(), 0}; }
    void close(PlanRange& r) const {
        r.unit1 = units.size();
        r.const1 = cfolds.size();
        r.slab1 = walk.slabs.size();
    }
    // The end of a batch whose work is independent in time (reduce_space, zonal, histogram): the last slab, the few-units split of
    // the batch's own units (plan_time_split: advance), the range.
    template <class F>
    void close_batch(PlanRange& r, uint32_t wanted, F&& advance) {
        walk.flush();
        plan_time_split(units, r.unit0, wanted, advance);
        close(r);
    }
};
// reduce_time and spells: within a time segment every cell of a cube lies in exactly one piece, so the work of one segment never
// shares a cell; the segments are launched one after the other in ascending order (ranges), and each piece continues the state its
// cells' planes hold.  The pieces are gathered per segment (put) and appended segment by segment (assemble).
using SegRange = PlanRange;
template <class Unit, class Fold>
struct SegmentPlan : ReducePlan<Unit, Fold> {
    std::vector<SegRange> ranges;
    using ReducePlan<Unit, Fold>::ReducePlan;
};
// The heads of a piece's records (k2r_cell_fold.h): piece p of a cube of wr x wc cells whose first output / scratch plane starts
// at base / sbase, and unit u of p.
K2R_PLAN_INLINE CellFold cell_fold(const PlanRaster& g, const Piece& p, uint64_t wr, uint64_t wc, uint64_t base, uint64_t sbase) {
    return CellFold{p.nt(), p.rows(), p.cols(), (uint32_t)wc, p.dt == 0 /* the piece holds the cube's first instant */, p.enc, p.fbits,
                    p.kind == PIECE_CONST, (uint64_t)p.leaf * g.cs + p.l.start, base + p.in_win, sbase + p.in_win, wr * wc};
}
template <class Unit>
K2R_PLAN_INLINE void cell_unit(Unit& u, const Piece& p, const CellFold& f) {
    u.sr = f.sr;
    u.init = f.init;
    u.o_off = f.o_off + unit_in_piece(u, p, f.sr);
    u.s_off = f.s_off + unit_in_piece(u, p, f.sr);
    u.psz = f.psz;
}
template <class Unit, class Fold>
struct SegmentBuckets {
    struct Segment {
        std::vector<Unit> units;
        std::vector<Fold> consts;
        std::vector<WalkPiece<Fold>> walks;
    };
    const uint32_t cs;
    std::vector<Segment> segs;
    explicit SegmentBuckets(const PlanRaster& g) : cs(g.cs), segs((g.T + g.cs - 1) / g.cs) {}
    // piece p with fold f into its segment; own(u) sets a bulk unit's own fields
    template <class F>
    K2R_PLAN_INLINE void put(const Piece& p, const Fold& f, F&& own) {
        Segment& S = segs[p.t0 / cs];
        if (p.kind == PIECE_CONST) S.consts.push_back(f);
        else if (p.kind == PIECE_WALK) S.walks.push_back(WalkPiece<Fold>{p.leaf, p.k, f});
        else plan_units(p, S.units, own);
    }
    // own(fold, a): SlabCutter::add_piece's, after init -- a part cut in time holds the cube's first instant only when it is the
    // piece's first
    template <class F>
    int assemble(SegmentPlan<Unit, Fold>& P, bool node_wise, F&& own) {
        for (Segment& S : segs) {
            if (S.units.empty() && S.consts.empty() && S.walks.empty()) continue;
            SegRange r = P.mark();
            P.units.insert(P.units.end(), S.units.begin(), S.units.end());
            P.cfolds.insert(P.cfolds.end(), S.consts.begin(), S.consts.end());
            for (const WalkPiece<Fold>& w : S.walks)
                P.walk.add_piece(w.chunk, w.k, w.f, node_wise, [&](Fold& f, uint32_t a) {
                    f.init = f.init && a == 0;
                    own(f, a);
                });
            P.walk.flush();  // (a slab never spans two segments)
            P.close(r);
            P.ranges.push_back(r);
            S = Segment{};
            if (P.full()) return DCDF_ERR_CAPACITY;
        }
        return DCDF_OK;
    }
};

// ---- decode ------------------------------------------------------------------------------------------------------------------
// base[q]: element of cube q's first cell in the output; all three lists write that one array
struct DecodePlan {
    std::vector<BulkUnit> units;
    std::vector<WinItem> items;
    std::vector<ConstPiece> consts;
    uint64_t stats[3] = {0, 0, 0};
};
inline int plan_decode(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, bool node_wise, uint32_t wanted,
                       DecodePlan& P) {
    P.units.reserve(plan_reserve(nq));
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if (cube_cells(c) == 0) continue;
        plan_pieces(g, c, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
            const uint64_t at = base[q] + p.dt * wr * wc + p.in_win;
            if (p.kind == PIECE_CONST) P.consts.push_back(ConstPiece{p.leaf, p.l.start, p.l.end, p.rows(), p.cols(), (uint32_t)wc, at, wr * wc});
            else if (p.kind == PIECE_WALK) window_items(p.leaf, p.k, at, P.items, node_wise, wc, wr * wc);
            else
                plan_units(p, P.units, [&](BulkUnit& u) {
                    u.out_sr = (uint32_t)wc;
                    u.out_st = wr * wc;
                    u.out_off = at + unit_in_piece(u, p, wc);
                });
        });
        if (P.units.size() > 0x3fffffffull || P.items.size() > 0xfffffff0ull || P.consts.size() > 0xfffffff0ull) return DCDF_ERR_CAPACITY;
    }
    plan_time_split(P.units, 0, wanted, [](BulkUnit& v, uint32_t dt) { v.out_off += (uint64_t)dt * v.out_st; });
    return DCDF_OK;
}

// ---- reduce over time --------------------------------------------------------------------------------------------------------
// A SegmentPlan: each piece continues the running sum of its cells' state plane.  base[q] / sbase[q]: cube q's first output /
// scratch plane.
struct TimePlan : SegmentPlan<ReduceUnit, FoldPiece> {
    std::vector<MeanPiece> means;
    using SegmentPlan::SegmentPlan;
};
inline int plan_reduce_time(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, const uint64_t* sbase, bool node_wise,
                            TimePlan& P) {
    SegmentBuckets<ReduceUnit, FoldPiece> B(g);
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if (cube_cells(c) == 0) continue;
        P.means.push_back(MeanPiece{base[q], sbase[q], wr * wc});
        plan_pieces(g, c, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
            const FoldPiece f = cell_fold(g, p, wr, wc, base[q], sbase[q]);
            B.put(p, f, [&](ReduceUnit& u) { cell_unit(u, p, f); });
        });
    }
    return B.assemble(P, node_wise, [](FoldPiece&, uint32_t) {});
}

// ---- grouped reduce over time ------------------------------------------------------------------------------------------------
// plan_reduce_time's plan with the accumulators' "planes" n_groups times as large (k2r_group.h): base[q] / sbase[q] are cube q's
// first output / scratch array [n_groups][rows][cols], loff[q] the place of its first label in the call's device label array.  No
// record initialises: k_group_fill sets the arrays `means` lists to the identities before the first segment.  A unit's instants are never
// split over workgroups (as in plan_spells): two workgroups on the same cells would have to merge a group's running sum.
struct GroupPlan : SegmentPlan<GroupUnit, GroupFold> {
    std::vector<MeanPiece> means;  // every cube's arrays: what the fill and MEAN run over
    using SegmentPlan::SegmentPlan;
};
inline int plan_reduce_time_groups(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* loff, uint32_t n_groups,
                                   const uint64_t* base, const uint64_t* sbase, bool node_wise, GroupPlan& P) {
    SegmentBuckets<GroupUnit, GroupFold> B(g);
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if (cube_cells(c) == 0) continue;
        P.means.push_back(MeanPiece{base[q], sbase[q], n_groups * wr * wc});
        plan_pieces(g, c, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
            GroupFold f{cell_fold(g, p, wr, wc, base[q], sbase[q]), loff[q] + p.dt, wr * wc};
            f.init = 0;
            f.psz = n_groups * wr * wc;
            B.put(p, f, [&](GroupUnit& u) {
                cell_unit(u, p, f);
                u.lab = f.lab;
                u.gsz = f.gsz;
            });
        });
    }
    return B.assemble(P, node_wise, [](GroupFold& f, uint32_t a) { f.lab += a; });  // a part cut in time: its own first label
}
// The call's device label array, as it is on the host: the labels of every cube that has cells -- its c.end - c.start instants,
// from labels[label_offset[q]] --, one cube after the other in batch order; loff[q]: the place of cube q's first (0 for a cube
// without cells).  labels == nullptr -- the ungrouped moments -- yields no label.
inline void gather_time_labels(const dcdf_cube* cubes, size_t nq, const uint16_t* labels, const uint64_t* label_offset, std::vector<uint64_t>& loff,
                               std::vector<uint16_t>& lab) {
    loff.assign(nq, 0);
    lab.clear();
    for (size_t q = 0; labels && q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (cube_cells(c) == 0) continue;
        loff[q] = lab.size();
        lab.insert(lab.end(), labels + label_offset[q], labels + label_offset[q] + (c.end - c.start));
    }
}

// ---- reduce over space -------------------------------------------------------------------------------------------------------
// Every piece leaves one SpacePartial per instant in a scratch array; the pieces of one (cube, segment) share their instants, so
// their records form one block [slot][instant] (a SpaceJob) that k_space_finish folds into the cube's series.  The jobs are
// taken in batches whose records fit rec_cap (a job beyond it alone: a huge cube's segment is cut in time first); the batches
// run one after the other over the same scratch.  base[q]: cube q's series; moff[q]: its mask's first byte.
struct SpaceBatch : PlanRange {
    size_t job0, job1;
    uint32_t job_nt;  // the longest job
};
struct SpacePlan : ReducePlan<SpaceUnit, SpaceFold> {
    std::vector<SpaceJob> jobs;
    std::vector<SpaceBatch> batches;
    uint64_t rec_max = 0;  // records of the largest batch
    using ReducePlan::ReducePlan;
};
inline int plan_reduce_space(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, const uint64_t* moff, bool node_wise,
                             uint64_t rec_cap, uint32_t wanted, SpacePlan& P) {
    uint64_t rec_used = 0;
    SpaceBatch cur{P.mark(), 0, 0, 0};
    P.units.reserve(plan_reserve(nq));
    P.jobs.reserve(plan_reserve(nq));
    auto flush_batch = [&] {
        // each part of a split unit writes its own instants' records
        P.close_batch(cur, wanted, [](SpaceUnit& v, uint32_t dt) { v.rec += dt; });
        cur.job1 = P.jobs.size();
        if (cur.job1 > cur.job0) P.batches.push_back(cur);
        P.rec_max = std::max(P.rec_max, rec_used);
        rec_used = 0;
        cur = SpaceBatch{P.mark(), P.jobs.size(), 0, 0};
    };
    std::vector<SpaceUnit> tu;  // the pieces of one (cube, segment), before they are cut into jobs
    std::vector<SpaceFold> tc;
    std::vector<WalkPiece<SpaceFold>> tw;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (c.end == c.start) continue;
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++) {
            const uint32_t s0 = seg * g.cs, ls = std::max(c.start, s0), le = std::min(c.end, s0 + g.cs);  // the cube's instants of this segment
            tu.clear();
            tc.clear();
            tw.clear();
            if (wr * wc != 0)
                plan_pieces(g, dcdf_cube{ls, le, c.top, c.bottom, c.left, c.right}, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
                    const SpaceFold f{p.nt(), p.rows(), p.cols(), (uint32_t)wc, p.enc, p.fbits, p.kind == PIECE_CONST, 0u,
                                      (uint64_t)p.leaf * g.cs + p.l.start, 0, moff[q] + p.in_win};
                    if (p.kind == PIECE_CONST) tc.push_back(f);
                    else if (p.kind == PIECE_WALK) tw.push_back(WalkPiece<SpaceFold>{p.leaf, p.k, f});
                    else
                        plan_units(p, tu, [&](SpaceUnit& u) {
                            u.m_sr = (uint32_t)wc;
                            u.m_off = f.m_off + unit_in_piece(u, p, wc);
                        });
                });
            // the segment's instants in jobs of at most rec_cap records (one job, but for a huge cube)
            const uint64_t n_slots = tu.size() + tc.size() + tw.size();
            const uint32_t nt = le - ls, step = n_slots ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, rec_cap / n_slots)) : nt;
            for (uint32_t a = 0; a < nt; a += step) {
                const uint32_t jn = std::min(nt, a + step) - a;
                if (rec_used && rec_used + n_slots * jn > rec_cap) flush_batch();
                P.jobs.push_back(SpaceJob{rec_used, (uint32_t)n_slots, jn, base[q] + (ls + a - c.start), (uint64_t)(c.end - c.start)});
                uint64_t rec = rec_used;  // a slot per piece: units, elided pieces, walk pieces
                for (SpaceUnit u : tu) {
                    u.t0 += a;
                    u.t1 = u.t0 + jn;
                    u.rec = rec;
                    P.units.push_back(u);
                    rec += jn;
                }
                for (SpaceFold f : tc) {
                    f.src += a;
                    f.nt = jn;
                    f.rec = rec;
                    P.cfolds.push_back(f);
                    rec += jn;
                }
                for (const WalkPiece<SpaceFold>& w : tw) {
                    P.walk.add_piece(w.chunk, cube_instants(w.k, a, a + jn), w.f, node_wise, [&](SpaceFold& f, uint32_t x) { f.rec = rec + x; });
                    rec += jn;
                }
                rec_used = rec;
                cur.job_nt = std::max(cur.job_nt, jn);
            }
            if (P.full() || P.jobs.size() > 0x7ffffff0ull) return DCDF_ERR_CAPACITY;
        }
    }
    flush_batch();
    return DCDF_OK;
}

// ---- zonal statistics ---------------------------------------------------------------------------------------------------------
// plan_reduce_space's pieces and units, without records and jobs: every piece adds to the accumulator entries of its cube's (zone,
// instant)s with integer atomics (k2r_zonal.h).  The entries -- ZONAL_BYTES each, n_zones per instant -- live in a scratch of at
// most acc_cap bytes: the cubes' instants are cut into spans, a batch takes spans while their entries fit (a single instant
// beyond the cap is a batch of its own), and the batches run one after the other over the same scratch: zero, accumulate, finish.
// base[q]: cube q's first matrix; moff[q]: its first label, in elements.
struct ZonalBatch : PlanRange {
    size_t span0, span1;
    uint64_t entries;
};
struct ZonalPlan : ReducePlan<ZonalUnit, ZonalFold> {
    std::vector<ZonalSpan> spans;
    std::vector<ZonalBatch> batches;
    uint64_t entries_max = 0;  // entries of the largest batch
    uint32_t span_nt = 1;      // the longest span
    using ReducePlan::ReducePlan;
};
inline int plan_zonal(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, const uint64_t* moff, uint32_t n_zones,
                      bool node_wise, uint64_t acc_cap, uint32_t wanted, ZonalPlan& P) {
    const uint64_t room = std::max<uint64_t>(1, acc_cap / (ZONAL_BYTES * n_zones));  // instants of one batch
    uint64_t used = 0;                                                                // instants of the current batch
    ZonalBatch cur{PlanRange{0, 0, 0, 0, 0, 0}, 0, 0, 0};
    P.units.reserve(plan_reserve(nq));
    P.spans.reserve(plan_reserve(nq));
    // (the batch end and the walk part are written out, not close_batch / add_piece: with those this function alone was 8 % slower)
    auto flush_batch = [&] {
        P.walk.flush();
        // each part of a split unit adds to its own instants' entries
        plan_time_split(P.units, cur.unit0, wanted, [](ZonalUnit& v, uint32_t dt) { v.acc += dt; });
        cur.unit1 = P.units.size();
        cur.const1 = P.cfolds.size();
        cur.slab1 = P.walk.slabs.size();
        cur.span1 = P.spans.size();
        cur.entries = used * n_zones;
        if (cur.span1 > cur.span0) P.batches.push_back(cur);
        P.entries_max = std::max(P.entries_max, cur.entries);
        used = 0;
        cur = ZonalBatch{PlanRange{P.units.size(), 0, P.cfolds.size(), 0, P.walk.slabs.size(), 0}, P.spans.size(), 0, 0};
    };
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint32_t NT = c.end - c.start;
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        for (uint32_t a = 0; a < NT;) {
            if (used == room) flush_batch();
            const uint32_t nt = (uint32_t)std::min<uint64_t>(NT - a, room - used);
            const uint64_t acc = used * n_zones;  // the span's entries: [zone][nt]
            P.spans.push_back(ZonalSpan{acc, nt, 0u, base[q] + a, (uint64_t)NT, (uint64_t)n_zones * NT});
            P.span_nt = std::max(P.span_nt, nt);
            if (wr * wc != 0)
                plan_pieces(g, dcdf_cube{c.start + a, c.start + a + nt, c.top, c.bottom, c.left, c.right}, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
                    const ZonalFold f{p.nt(), p.rows(), p.cols(), (uint32_t)wc, p.enc, p.fbits, p.kind == PIECE_CONST, nt,
                                      (uint64_t)p.leaf * g.cs + p.l.start, acc + p.dt, moff[q] + p.in_win};
                    if (p.kind == PIECE_CONST) {
                        P.cfolds.push_back(f);
                    } else if (p.kind == PIECE_WALK) {
                        P.walk.add(f.nt, (uint64_t)f.rows * f.cols, [&](uint32_t x, uint32_t y, uint64_t src) {
                            ZonalFold w = f;
                            w.nt = y - x;
                            w.src = src;
                            w.acc = f.acc + x;
                            window_items(p.leaf, cube_instants(p.k, x, y), src, P.walk.items, node_wise);
                            P.walk.folds.push_back(w);
                        });
                    } else {
                        plan_units(p, P.units, [&](ZonalUnit& u) {
                            u.m_sr = (uint32_t)wc;
                            u.a_st = nt;
                            u.acc = f.acc;
                            u.m_off = f.m_off + unit_in_piece(u, p, wc);
                        });
                    }
                });
            used += nt;
            a += nt;
            if (P.units.size() > 0x3fffffffull || P.walk.items.size() > 0xfffffff0ull || P.cfolds.size() + P.walk.folds.size() > 0xfffffff0ull ||
                P.spans.size() > 0x7ffffff0ull)
                return DCDF_ERR_CAPACITY;
        }
    }
    flush_batch();
    return DCDF_OK;
}

// ---- histogram ---------------------------------------------------------------------------------------------------------------
// Every piece adds its counts to the cube's own [instants][bins] array (base[q]) with integer atomics, so the work of all
// segments and cubes goes into one launch of each kind.  thr: the thresholds of every distinct (encoding, fractional bits) among
// the bulk kernel's leaves (hist_thresholds32), 2^hist_steps(n_bins) entries each, translated once.
struct HistPlan : ReducePlan<HistUnit, HistFold> {
    std::vector<int32_t> thr;
    using ReducePlan::ReducePlan;
};
inline int plan_histogram(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, const uint64_t* moff, const double* edges,
                          uint32_t n_bins, bool node_wise, uint32_t wanted, HistPlan& P) {
    const uint32_t tab = (uint32_t)1 << hist_steps(n_bins);
    std::map<std::pair<int32_t, uint32_t>, uint32_t> leaf_thr;
    P.units.reserve(plan_reserve(nq));
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wc = c.right - c.left;
        if (cube_cells(c) == 0) continue;
        plan_pieces(g, c, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
            const HistFold f{p.nt(), p.rows(), p.cols(), (uint32_t)wc, p.enc, p.fbits, p.kind == PIECE_CONST, 0u,
                             (uint64_t)p.leaf * g.cs + p.l.start, base[q] + (uint64_t)p.dt * n_bins, moff[q] + p.in_win};
            if (p.kind == PIECE_CONST) {
                P.cfolds.push_back(f);
            } else if (p.kind == PIECE_WALK) {
                P.walk.add_piece(p.leaf, p.k, f, node_wise, [&](HistFold& w, uint32_t x) { w.o_off += (uint64_t)x * n_bins; });
            } else {
                auto it = leaf_thr.find({p.enc, p.fbits});
                if (it == leaf_thr.end()) {
                    it = leaf_thr.emplace(std::make_pair(p.enc, p.fbits), (uint32_t)P.thr.size()).first;
                    P.thr.resize(P.thr.size() + tab);
                    hist_thresholds32(p.enc, p.fbits, edges, n_bins, P.thr.data() + it->second, tab);
                }
                plan_units(p, P.units, [&](HistUnit& u) {
                    u.m_sr = (uint32_t)wc;
                    u.thr = it->second;
                    u.rev = hist_reversed(p.enc, p.fbits) ? 1u : 0u;
                    u.o_off = f.o_off;
                    u.m_off = f.m_off + unit_in_piece(u, p, wc);
                });
            }
        });
        if (P.full() || P.thr.size() > 0x7fffffffull) return DCDF_ERR_CAPACITY;
    }
    // one batch; each part of a split unit adds to its own instants' rows
    PlanRange all{};
    P.close_batch(all, wanted, [n_bins](HistUnit& v, uint32_t dt) { v.o_off += (uint64_t)dt * n_bins; });
    return DCDF_OK;
}

// ---- spell statistics --------------------------------------------------------------------------------------------------------
// A SegmentPlan: each piece continues the run state its cells' planes hold.  A unit's instants are never split over workgroups (no
// plan_time_split): two workgroups on the same cells would have to merge runs.  lower[q] / upper[q] are translated once per
// (cube, encoding, fractional bits) into the leaf's stored integers (value_bounds).  base[q] / sbase[q]: cube q's first output /
// scratch plane.
using SpellPlan = SegmentPlan<SpellUnit, SpellFold>;
inline int plan_spells(const PlanRaster& g, const dcdf_cube* cubes, const double* lower, const double* upper, size_t nq, const uint64_t* base,
                       const uint64_t* sbase, bool node_wise, SpellPlan& P) {
    struct LeafRange {
        int32_t enc;
        uint32_t fbits;
        ValueRange vr;
    };
    SegmentBuckets<SpellUnit, SpellFold> B(g);
    std::vector<LeafRange> cache;  // of one cube: a raster has few distinct (encoding, fractional bits)
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        if (lower[q] != lower[q] || upper[q] != upper[q]) return DCDF_ERR_BAD_ARG;
        if (cube_cells(c) == 0) continue;
        cache.clear();
        bool bad = false;
        plan_pieces(g, c, P.stats, [&](const Piece& p) K2R_PLAN_LAMBDA {
            size_t at = 0;
            while (at < cache.size() && (cache[at].enc != p.enc || cache[at].fbits != p.fbits)) at++;
            if (at == cache.size()) {
                cache.push_back(LeafRange{p.enc, p.fbits, ValueRange{}});
                if (!value_bounds(p.enc, p.fbits, lower[q], upper[q], &cache[at].vr)) bad = true;
            }
            const ValueRange& vr = cache[at].vr;
            const SpellRange64 r64 = spell_range64(vr);
            const SpellFold f{cell_fold(g, p, wr, wc, base[q], sbase[q]), p.dt, r64.flags, r64.lo, r64.hi};
            const SpellRange32 r32 = p.kind == PIECE_BULK ? spell_range32(vr) : SpellRange32{};  // the units' alone
            B.put(p, f, [&](SpellUnit& u) {
                cell_unit(u, p, f);
                u.dt = p.dt;
                u.lo = r32.lo;
                u.hi = r32.hi;
                u.flags = r32.flags;
            });
        });
        if (bad) return DCDF_ERR_BAD_ARG;
    }
    return B.assemble(P, node_wise, [](SpellFold& f, uint32_t a) { f.dt += a; });  // a part cut in time: its own first instant
}

// ---- quantiles over time -----------------------------------------------------------------------------------------------------
// Selection needs all of a cell's values at once, so the cubes are decoded, band by band, into a bounded slab of stored integers
// that k_quantile_select then reads.  A column is the part of a cube inside one leaf's place of the grid, over all the cube's
// instants -- so within a segment all its cells are widened alike (QuantileSeg) --, cut further on multiples of 64 raster rows and
// columns while its slab would exceed cap_bytes.  A band takes columns while their slabs fit (a column beyond the cap alone: the
// cap bounds batching, not correctness).  Each band is a batch of sub-cubes for plan_decode, their bases inside the slab and the
// output type DCDF_I64: bulk units, the walk's items and elided fills all land there by the kernels decode uses.  The bands'
// lists lie one after the other; the bands run one after the other over the same slab.  base[q]: cube q's first output plane.
struct QuantileBand {
    size_t col0, col1, unit0, unit1, item0, item1, const0, const1;
    uint64_t max_cells;  // of its largest column
};
struct QuantilePlan {
    std::vector<QuantileCol> cols;
    std::vector<QuantileSeg> segs;
    std::vector<uint32_t> col_cube;  // the cube of every column (the selection does not ask; plan_regress_time does)
    std::vector<BulkUnit> units;
    std::vector<WinItem> items;
    std::vector<ConstPiece> consts;
    std::vector<QuantileBand> bands;
    uint64_t slab_max = 0;  // elements of the largest band's slab
    uint64_t stats[3] = {0, 0, 0};
};
inline int plan_quantile_time(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, uint64_t cap_bytes, bool node_wise,
                              uint32_t wanted, QuantilePlan& P) {
    const uint64_t cap = std::max<uint64_t>(1, cap_bytes / sizeof(int64_t));  // elements
    std::vector<dcdf_cube> subs;  // the current band's columns as cubes of their own, and where each starts in the slab
    std::vector<uint64_t> sbase;
    uint64_t used = 0;
    QuantileBand cur{0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto flush = [&]() -> int {
        if (subs.empty()) return DCDF_OK;
        DecodePlan D;
        const int rc = plan_decode(g, subs.data(), subs.size(), sbase.data(), node_wise, wanted, D);
        if (rc != DCDF_OK) return rc;
        P.units.insert(P.units.end(), D.units.begin(), D.units.end());
        P.items.insert(P.items.end(), D.items.begin(), D.items.end());
        P.consts.insert(P.consts.end(), D.consts.begin(), D.consts.end());
        for (int k = 0; k < 3; k++) P.stats[k] += D.stats[k];
        cur.col1 = P.cols.size();
        cur.unit1 = P.units.size();
        cur.item1 = P.items.size();
        cur.const1 = P.consts.size();
        P.bands.push_back(cur);
        P.slab_max = std::max(P.slab_max, used);
        cur = QuantileBand{cur.col1, 0, cur.unit1, 0, cur.item1, 0, cur.const1, 0, 0};
        subs.clear();
        sbase.clear();
        used = 0;
        return DCDF_OK;
    };
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (cube_cells(c) == 0) continue;
        const uint32_t nt = c.end - c.start;
        const uint64_t wr = c.bottom - c.top, wc = c.right - c.left;
        for (uint32_t ti = c.top / g.tile; ti <= (c.bottom - 1) / g.tile; ti++)
            for (uint32_t tj = c.left / g.tile; tj <= (c.right - 1) / g.tile; tj++) {
                const uint32_t top = std::max(c.top, ti * g.tile), bottom = std::min(c.bottom, (ti + 1) * g.tile);
                const uint32_t left = std::max(c.left, tj * g.tile), right = std::min(c.right, (tj + 1) * g.tile);
                // the column's table: one entry per segment the cube meets
                const uint32_t seg0 = (uint32_t)P.segs.size();
                for (uint32_t seg = c.start / g.cs; seg <= (c.end - 1) / g.cs; seg++) {
                    const PlanLeaf& L = g.leaves[((uint64_t)seg * g.nti + ti) * g.ntj + tj];
                    P.segs.push_back(QuantileSeg{std::max(c.start, seg * g.cs) - c.start, L.enc, L.fbits});
                }
                const uint32_t nseg = (uint32_t)P.segs.size() - seg0;
                // rows and columns of a part: whole while the slab fits, else multiples of 64 (at least 64)
                const uint64_t fit = cap / nt;  // cells
                uint32_t pr = bottom - top, pc = right - left;
                if ((uint64_t)pr * pc > fit) {
                    pr = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(pr, fit / pc) / 64 * 64);
                    if ((uint64_t)pr * pc > fit) pc = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(pc, fit / pr) / 64 * 64);
                }
                for (uint32_t r0 = top; r0 < bottom;) {
                    const uint32_t r1 = std::min(bottom, pr >= bottom - top ? bottom : r0 / 64 * 64 + pr);
                    for (uint32_t c0 = left; c0 < right;) {
                        const uint32_t c1 = std::min(right, pc >= right - left ? right : c0 / 64 * 64 + pc);
                        const uint64_t cells = (uint64_t)(r1 - r0) * (c1 - c0), need = cells * nt;
                        if (used && used + need > cap) {
                            const int rc = flush();
                            if (rc != DCDF_OK) return rc;
                        }
                        P.cols.push_back(QuantileCol{nt, r1 - r0, c1 - c0, (uint32_t)wc, seg0, nseg, used,
                                                     base[q] + (uint64_t)(r0 - c.top) * wc + (c0 - c.left), wr * wc});
                        P.col_cube.push_back((uint32_t)q);
                        subs.push_back(dcdf_cube{c.start, c.end, r0, r1, c0, c1});
                        sbase.push_back(used);
                        used += need;
                        cur.max_cells = std::max(cur.max_cells, cells);
                        c0 = c1;
                    }
                    r0 = r1;
                }
                if (P.cols.size() > 0x7ffffff0ull || P.segs.size() > 0x7ffffff0ull) return DCDF_ERR_CAPACITY;
            }
    }
    return flush();
}

// ---- regression over time ----------------------------------------------------------------------------------------------------
// The cubes are decoded exactly as for the quantiles -- plan_quantile_time's bands, columns, segment tables, units, items and
// elided fills over a slab of cap_bytes --, and k_regress_stream reads every cell's series from the slab once.  What it needs
// beside a column is made here per cube that has cells (k2r_regress.h): the records of the instants that belong to a group, sorted
// by (label, instant) -- a counting sort, stable, so a group's instants stay in order --, and the CSR of the groups over them,
// counted from the cube's first record.  labels == nullptr: the ungrouped call, one group (n_groups == 1) of every instant in
// order.  regressor == nullptr: the instant index counted from the cube's first instant.  A regressor value that is not finite
// anywhere in the array of a cube that has cells: DCDF_ERR_BAD_ARG.  base[q]: cube q's first output plane.
struct RegressPlan {
    QuantilePlan q;
    std::vector<RegressCol> cols;  // q.cols with their cube's rec0, start0
    std::vector<RegressRec> recs;
    std::vector<uint32_t> start;   // n_groups + 1 per cube that has cells
};
inline int plan_regress_time(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, uint64_t cap_bytes, bool node_wise,
                             uint32_t wanted, const double* regressor, const uint64_t* regressor_offset, const uint16_t* labels,
                             const uint64_t* label_offset, uint32_t n_groups, RegressPlan& P) {
    std::vector<uint32_t> rec0(nq, 0), start0(nq, 0), fill;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (cube_cells(c) == 0) continue;
        const uint32_t nt = c.end - c.start;
        const double* const e = regressor ? regressor + regressor_offset[q] : nullptr;
        const uint16_t* const lab = labels ? labels + label_offset[q] : nullptr;
        for (uint32_t t = 0; e && t < nt; t++)
            if (!regress_finite(e[t])) return DCDF_ERR_BAD_ARG;
        if (P.recs.size() + nt > 0x7ffffff0ull || P.start.size() + n_groups + 1ull > 0x7ffffff0ull) return DCDF_ERR_CAPACITY;
        rec0[q] = (uint32_t)P.recs.size();
        start0[q] = (uint32_t)P.start.size();
        // the groups' sizes, then their first records, then every instant into its group's next place
        P.start.resize(P.start.size() + n_groups + 1u, 0u);
        uint32_t* const st = P.start.data() + start0[q];
        for (uint32_t t = 0; t < nt; t++) {
            const uint32_t l = lab ? lab[t] : 0u;
            if (l != 0xffffu && l < n_groups) st[l + 1u]++;
        }
        for (uint32_t l = 0; l < n_groups; l++) st[l + 1u] += st[l];
        P.recs.resize(P.recs.size() + st[n_groups]);
        RegressRec* const rec = P.recs.data() + rec0[q];
        fill.assign(st, st + n_groups);
        for (uint32_t t = 0; t < nt; t++) {
            const uint32_t l = lab ? lab[t] : 0u;
            if (l == 0xffffu || l >= n_groups) continue;
            rec[fill[l]++] = RegressRec{e ? e[t] : (double)t, t, (c.start + t) / g.cs - c.start / g.cs};
        }
    }
    const int rc = plan_quantile_time(g, cubes, nq, base, cap_bytes, node_wise, wanted, P.q);
    if (rc != DCDF_OK) return rc;
    P.cols.reserve(P.q.cols.size());
    for (size_t i = 0; i < P.q.cols.size(); i++) P.cols.push_back(RegressCol{P.q.cols[i], rec0[P.q.col_cube[i]], start0[P.q.col_cube[i]]});
    return DCDF_OK;
}

// ---- rolling windows over time --------------------------------------------------------------------------------------------------
// The cubes are decoded exactly as for the quantiles and the regression -- plan_quantile_time's bands, columns, segment tables,
// units, items and elided fills over a slab of cap_bytes --, and k_rolling_stream reads every cell's series from the slab.  What it
// needs beside a column is made here per cube that has cells (k2r_rolling.h): seg_of, the segment-table entry of EVERY instant of
// the cube (a window reaches back over instants of any label); ends, the instants i >= window - 1 that belong to a group, sorted
// by (label, instant) -- a counting sort, stable, so a group's instants stay ascending --; and the CSR of the groups over them,
// counted from the cube's first.  labels == nullptr: the plain call, one group (n_groups == 1) of every window.  The call's own
// arguments are refused before anything is made.  base[q]: cube q's first output plane.
struct RollingPlan {
    QuantilePlan q;
    std::vector<RollingCol> cols;  // q.cols with their cube's end0, start0, seg_of0
    std::vector<uint32_t> ends;
    std::vector<uint32_t> start;   // n_groups + 1 per cube that has cells
    std::vector<uint32_t> seg_of;  // its instants per cube that has cells
};
inline int plan_rolling_time(const PlanRaster& g, const dcdf_cube* cubes, size_t nq, const uint64_t* base, uint64_t cap_bytes, bool node_wise,
                             uint32_t wanted, uint32_t ops, uint32_t window, uint32_t min_count, int32_t kind, const uint16_t* labels,
                             const uint64_t* label_offset, uint32_t n_groups, RollingPlan& P) {
    if (!rolling_args_ok(ops, window, min_count, kind) || n_groups < 1u || n_groups > 65535u) return DCDF_ERR_BAD_ARG;
    std::vector<uint32_t> end0(nq, 0), start0(nq, 0), seg_of0(nq, 0), fill;
    for (size_t q = 0; q < nq; q++) {
        const dcdf_cube c = norm_cube(cubes[q]);
        if (cube_cells(c) == 0) continue;
        const uint32_t nt = c.end - c.start;
        const uint16_t* const lab = labels ? labels + label_offset[q] : nullptr;
        if (P.ends.size() + nt > 0x7ffffff0ull || P.start.size() + n_groups + 1ull > 0x7ffffff0ull) return DCDF_ERR_CAPACITY;
        end0[q] = (uint32_t)P.ends.size();
        start0[q] = (uint32_t)P.start.size();
        seg_of0[q] = (uint32_t)P.seg_of.size();
        for (uint32_t t = 0; t < nt; t++) P.seg_of.push_back((c.start + t) / g.cs - c.start / g.cs);
        // the groups' sizes, then their first windows, then every window's end into its group's next place
        P.start.resize(P.start.size() + n_groups + 1u, 0u);
        uint32_t* const st = P.start.data() + start0[q];
        for (uint32_t t = window - 1u; t < nt; t++) {
            const uint32_t l = lab ? lab[t] : 0u;
            if (l != 0xffffu && l < n_groups) st[l + 1u]++;
        }
        for (uint32_t l = 0; l < n_groups; l++) st[l + 1u] += st[l];
        P.ends.resize(P.ends.size() + st[n_groups]);
        uint32_t* const end = P.ends.data() + end0[q];
        fill.assign(st, st + n_groups);
        for (uint32_t t = window - 1u; t < nt; t++) {
            const uint32_t l = lab ? lab[t] : 0u;
            if (l == 0xffffu || l >= n_groups) continue;
            end[fill[l]++] = t;
        }
    }
    const int rc = plan_quantile_time(g, cubes, nq, base, cap_bytes, node_wise, wanted, P.q);
    if (rc != DCDF_OK) return rc;
    P.cols.reserve(P.q.cols.size());
    for (size_t i = 0; i < P.q.cols.size(); i++) {
        const uint32_t q = P.q.col_cube[i];
        P.cols.push_back(RollingCol{P.q.cols[i], end0[q], start0[q], seg_of0[q], 0u});
    }
    return DCDF_OK;
}

#undef K2R_PLAN_INLINE
#undef K2R_PLAN_LAMBDA

}  // namespace k2r
