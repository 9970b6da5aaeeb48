// k2r_group.h -- grouped reduction over time (dcdf_raster_reduce_time_groups_batch): what the planner (k2r_plan.h), the bulk
// kernel (k2r_bulk.hip) and the fold kernel (k2r_raster_region.hip) share.  Compiles for the host alone as well (g++).
//
// The contract (include/dcdf_k2r.h): reduce_time's five statistics (k2r_reduce.h), per cell, separately for
// every group of a per-instant label array: instant i of a cube belongs to group labels[i] when that is < n_groups, else to none.
// Accumulator A of a cube is one array [n_groups][rows][cols] -- state_plane's "plane", psz = n_groups * gsz --, group g sits
// g * gsz into it.  Every such array is filled with the identities (SUM 0.0, COUNT 0, MIN / MAX NaN) before the first segment
// (k_group_fill), so no piece tells a group's first touch from a later one: every piece loads, none initialises.  A piece walks
// its instants once, in order; on a change of group it merges what it gathered into the old group's planes and takes up the new
// group's running sum (group_step), so per cell and group the chain s = s + x[t] is the sequential one whatever the cut.
#pragma once
#include <cmath>

#include "k2r_reduce.h"

namespace k2r {

constexpr uint32_t GROUP_NONE = 0xffffu;  // DCDF_GROUP_NONE; every label >= n_groups is treated alike

// One workgroup's work in k_bulk_group: ReduceUnit, then where the label of instant t0 sits in the call's device label array and
// the cells of one group plane.  (init is never set: the planes are filled first.)
struct GroupUnit : ReduceUnit {
    uint64_t lab, gsz;
};
// A fallback or elided piece: the shared head, then the same two fields.
struct GroupFold : CellFold {
    uint64_t lab, gsz;
};
K2R_PIN_BEGIN
static_assert(sizeof(GroupUnit) == 72 && sizeof(GroupFold) == 80, "GroupUnit, GroupFold");
K2R_PIN(GroupUnit, psz, 48) K2R_PIN(GroupUnit, lab, 56) K2R_PIN(GroupUnit, gsz, 64)
K2R_PIN(GroupFold, psz, 56) K2R_PIN(GroupFold, lab, 64) K2R_PIN(GroupFold, gsz, 72)
K2R_PIN_END

// One cell's state while a piece walks its instants: the accumulators of the run of group g (GROUP_NONE: no run is open).
struct GroupState {
    double s, c, lo, hi;
    uint32_t g;
};
K2R_HD GroupState group_init() { return GroupState{0.0, 0.0, __builtin_nan(""), __builtin_nan(""), GROUP_NONE}; }
// The planes of one cell: element (group 0, the cell) of every live accumulator (nullptr when not live); group g is g * gsz on.
struct GroupPlanes {
    double *p_min, *p_max, *p_sum, *p_cnt;
    uint64_t gsz;
};
// the open run into its group's planes: SUM stored (the run began with the plane's value), COUNT added, MIN / MAX by fmin / fmax
K2R_HD void group_merge(const GroupState& st, const GroupPlanes& P) {
    if (st.g == GROUP_NONE) return;
    const uint64_t at = (uint64_t)st.g * P.gsz;
    if (P.p_sum) P.p_sum[at] = st.s;
    if (P.p_cnt) P.p_cnt[at] = P.p_cnt[at] + st.c;
    if (P.p_min) P.p_min[at] = fmin(P.p_min[at], st.lo);
    if (P.p_max) P.p_max[at] = fmax(P.p_max[at], st.hi);
}
// One instant with label `label` and value x (reduce_widen's) into the state.  An instant of no group changes nothing.
K2R_HD void group_step(GroupState& st, const GroupPlanes& P, uint32_t label, uint32_t n_groups, double x) {
    if (label >= n_groups) return;
    if (label != st.g) {
        group_merge(st, P);
        st = group_init();
        st.g = label;
        if (P.p_sum) st.s = P.p_sum[(uint64_t)label * P.gsz];
    }
    if (x == x) {
        st.s = st.s + x;
        st.c = st.c + 1.0;
        st.lo = fmin(st.lo, x);
        st.hi = fmax(st.hi, x);
    }
}

#if defined(__HIPCC__)
struct ChunkRef;
// k_bulk_group over n units on the null stream (asynchronous).  d_enc: the chunks' encodings; d_labels: the call's labels.
// Returns a DCDF code.
int launch_bulk_group(const ChunkRef* d_refs, const uint8_t* d_enc, const GroupUnit* d_units, uint32_t n, const uint16_t* d_labels,
                      uint32_t n_groups, double* d_dst, double* d_scr, uint32_t ops);
#endif

}  // namespace k2r
