// k2r_spell.h -- spell statistics over time (dcdf_raster_spells_batch): what the planner (k2r_plan.h), the bulk kernel
// (k2r_bulk.hip), the fold kernel (k2r_raster_region.hip) and the CPU check (tests/sim/spell_check.cpp) share.  Compiles for the
// host alone as well (g++).
//
// The contract (include/dcdf_k2r.h): instant i of a cell, counted from its cube's first instant, is a HIT
// iff the cell's stored integer lies in the set value_bounds (k2r_decode.h) gives for the leaf's encoding and fractional bits.
// Per cell, over i ascending, with cur = the length of the run of hits that ends at i: COUNT = the hits, LONGEST = the largest cur,
// LONGEST_START = the i at which the first run of that length began, FIRST / LAST = the first / last i that hit.  All of it is one
// sequential fold with a state of six integers (spell_step); a piece of the plan loads the state its predecessor stored, so the
// result depends on no cut of a cell's instants.
#pragma once
#include "k2r_cell_fold.h"

namespace k2r {

// the DCDF_SPELL_* bits, and SP_CUR: the run that ends at the last instant folded so far -- state only, never an output
constexpr uint32_t SP_COUNT = 1u, SP_LONGEST = 2u, SP_LSTART = 4u, SP_FIRST = 8u, SP_LAST = 16u, SP_ALL = 31u, SP_CUR = 32u;
constexpr uint32_t SPELL_NONE = 0xffffffffu;
// the state a call carries: LONGEST_START changes when cur > longest, so it needs LONGEST, and both need cur
K2R_HD uint32_t spell_live(uint32_t ops) {
    ops &= SP_ALL;
    if (ops & SP_LSTART) ops |= SP_LONGEST;
    if (ops & SP_LONGEST) ops |= SP_CUR;
    return ops;
}
// the three groups the bulk kernel is instantiated over
constexpr uint32_t SG_COUNT = 1u, SG_RUNS = 2u, SG_ENDS = 4u;
K2R_HD uint32_t spell_groups(uint32_t ops) {
    return ((ops & SP_COUNT) ? SG_COUNT : 0u) | ((ops & (SP_LONGEST | SP_LSTART)) ? SG_RUNS : 0u) | ((ops & (SP_FIRST | SP_LAST)) ? SG_ENDS : 0u);
}

// Where state A of a cube lives (state_plane, k2r_cell_fold.h): cur, and LONGEST kept for LONGEST_START alone, are the scratch
// planes.
K2R_HD uint32_t* spell_plane(uint32_t A, uint32_t* dst, uint32_t* scr, uint32_t ops, uint64_t o_off, uint64_t s_off, uint64_t psz) {
    return state_plane(A, spell_live(ops), dst, scr, ops, o_off, s_off, psz);
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------
struct SpellState {
    uint32_t count, cur, longest, lstart, first, last;
};
K2R_HD SpellState spell_init() { return SpellState{0u, 0u, 0u, SPELL_NONE, SPELL_NONE, SPELL_NONE}; }
// One instant: i counts from the cube's first instant.  Written without branches (selects): a miss leaves cur = 0, which never
// exceeds longest, so the run state only moves on a hit; on ties the earliest run stays.
K2R_HD void spell_step(SpellState& s, uint32_t i, bool hit) {
    s.cur = hit ? s.cur + 1u : 0u;
    s.count += hit ? 1u : 0u;
    const bool up = s.cur > s.longest;
    s.lstart = up ? i + 1u - s.cur : s.lstart;
    s.longest = up ? s.cur : s.longest;
    s.first = hit && s.first == SPELL_NONE ? i : s.first;
    s.last = hit ? i : s.last;
}

// ---- the hit test ------------------------------------------------------------------------------------------------------------
// A leaf's set of hits: [lo, hi] less 0 when SH_HOLE; nothing at all when SH_EMPTY (never encoded in lo / hi alone).
constexpr uint32_t SH_HOLE = 1u, SH_EMPTY = 2u;
struct SpellRange64 {
    int64_t lo, hi;
    uint32_t flags;
};
struct SpellRange32 {
    int32_t lo, hi;
    uint32_t flags;
};
K2R_HD SpellRange64 spell_range64(const ValueRange& v) {
    if (v.empty || v.lo > v.hi) return SpellRange64{0, 0, SH_EMPTY};
    return SpellRange64{v.lo, v.hi, v.hole ? SH_HOLE : 0u};
}
// The bulk kernel only sees narrow32 chunks: every stored value lies in [-2^30, 2^30), so clamping the range to int32 changes no
// answer; a range wholly beyond int32 is empty.
K2R_HD SpellRange32 spell_range32(const ValueRange& v) {
    if (v.empty || v.lo > v.hi || v.lo > (int64_t)INT32_MAX || v.hi < (int64_t)INT32_MIN) return SpellRange32{0, 0, SH_EMPTY};
    return SpellRange32{v.lo < (int64_t)INT32_MIN ? INT32_MIN : (int32_t)v.lo, v.hi > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)v.hi,
                        v.hole ? SH_HOLE : 0u};
}
// two signed compares, the hole, the flag: integer compares only, nothing is widened
K2R_HD bool spell_hit32(int32_t n, int32_t lo, int32_t hi, uint32_t flags) {
    return n >= lo && n <= hi && !((flags & SH_HOLE) != 0 && n == 0) && (flags & SH_EMPTY) == 0;
}
K2R_HD bool spell_hit64(int64_t n, int64_t lo, int64_t hi, uint32_t flags) {
    return n >= lo && n <= hi && !((flags & SH_HOLE) != 0 && n == 0) && (flags & SH_EMPTY) == 0;
}

// ---- the plan's records ------------------------------------------------------------------------------------------------------
// One workgroup's work in k_bulk_spell: CellUnit (k2r_cell_fold.h), the leaf's range, then the place of its cells in the state
// planes.  dt: the index of t0 counted from the cube's first instant.
struct SpellUnit : CellUnit {
    uint32_t dt;
    int32_t lo, hi;  // spell_range32 of the leaf
    uint32_t flags;
    uint64_t o_off, s_off, psz;  // of cell (top, left): spell_plane
};
// A fallback or elided piece: CellFold with dt and the leaf's range as stored integers.
struct SpellFold : CellFold {
    uint32_t dt, flags;
    int64_t lo, hi;
};
K2R_PIN_BEGIN
static_assert(sizeof(SpellUnit) == 72 && sizeof(SpellFold) == 88, "SpellUnit, SpellFold");
K2R_PIN(SpellUnit, init, 28) K2R_PIN(SpellUnit, dt, 32) K2R_PIN(SpellUnit, lo, 36) K2R_PIN(SpellUnit, hi, 40) K2R_PIN(SpellUnit, flags, 44)
K2R_PIN(SpellUnit, o_off, 48) K2R_PIN(SpellUnit, s_off, 56) K2R_PIN(SpellUnit, psz, 64)
K2R_PIN(SpellFold, psz, 56) K2R_PIN(SpellFold, dt, 64) K2R_PIN(SpellFold, flags, 68) K2R_PIN(SpellFold, lo, 72) K2R_PIN(SpellFold, hi, 80)
K2R_PIN_END

#if defined(__HIPCC__)
struct ChunkRef;
// k_bulk_spell over n units on the null stream (asynchronous).  Returns a DCDF code.
int launch_bulk_spell(const ChunkRef* d_refs, const SpellUnit* d_units, uint32_t n, uint32_t* d_dst, uint32_t* d_scr, uint32_t ops);
#endif

}  // namespace k2r
