// k2r_moment.h -- moments over time (dcdf_raster_moments_time_batch, dcdf_raster_moments_time_groups_batch, dcdf_moments_host):
// what the bulk kernel (k2r_bulk.hip), the fold kernel and the entry points (k2r_raster_region.hip) share.  Compiles for the
// host alone as well (g++).
//
// The contract (include/dcdf_k2r.h): per cell -- and per group of a per-instant label array, k2r_group.h --
// the state is four doubles (c, K, s1, s2), at first (0, NaN, +0.0, +0.0).  In instant order every non-NaN x[t] (reduce_widen's)
// does  if (c == 0) K = x;  d = x - K;  s1 = s1 + d;  s2 = s2 + d * d;  c = c + 1  -- each one IEEE double operation, nothing
// contracted into an fma (moment_step).  K, the shift, is the series' first value: a sample of the series, so (mean - K)^2 / VAR
// <= n and the shifted textbook formula keeps a relative error of VAR of order (n + 2)^2 * 2^-53.  Finishing (moment_finish):
// COUNT = c, m = s1 / c, MEAN = K + m, q = max(s2 - s1 * m, +0.0), VAR = q / (c - ddof) when c > ddof else NaN, STD = sqrt(VAR)
// correctly rounded.  Consequences: a constant series has VAR exactly +0.0 and MEAN exactly its value; one value with ddof = 1
// gives NaN; MEAN may differ from SUM / COUNT in the last bits; for integer leaves with |x| < 2^53 a constant added to every
// value leaves VAR and STD unchanged bit for bit (every d is exact).
//
// The state is loaded and stored whole -- there is no merge rule --, so the plan is the grouped reduce's as it is (GroupPlan,
// GroupUnit, GroupFold): the four state arrays [n_groups][rows][cols] of a cube are filled with the identities before the first
// segment, every piece loads, none initialises, and the ungrouped call is one group with no label array (moment_label).
#pragma once
#include <cmath>

#include "k2r_group.h"

namespace k2r {

// the statistics (DCDF_MOMENT_*), in plane order
constexpr uint32_t MO_COUNT = 1u, MO_MEAN = 2u, MO_VAR = 4u, MO_STD = 8u, MO_ALL = 15u;
// The states, for state_plane (k2r_cell_fold.h): COUNT's state is its output plane when asked for; K, s1, s2 -- bits above every
// statistic's -- and an unrequested COUNT are scratch planes.  MEAN, VAR and STD are no states: the finishing kernel alone writes
// them, each to the output plane state_plane gives for its own bit.
constexpr uint32_t MS_COUNT = MO_COUNT, MS_K = 16u, MS_S1 = 32u, MS_S2 = 64u, MS_ALL = MS_COUNT | MS_K | MS_S1 | MS_S2;
K2R_HD double* moment_plane(uint32_t A, double* dst, double* scr, uint32_t ops, uint64_t o_off, uint64_t s_off, uint64_t psz) {
    return state_plane(A, MS_ALL, dst, scr, ops, o_off, s_off, psz);
}

#if defined(__clang__)
#define K2R_FP_STRICT _Pragma("clang fp contract(off)")
#define K2R_FP_STRICT_FN
#else
#define K2R_FP_STRICT
#define K2R_FP_STRICT_FN __attribute__((optimize("fp-contract=off")))
#endif

struct MomentState {
    double c, K, s1, s2;
};
K2R_HD MomentState moment_init() { return MomentState{0.0, __builtin_nan(""), 0.0, 0.0}; }

// One value into a state; a NaN changes nothing.  Written with selects, not branches: the bulk kernel runs it on 16 cells per
// thread and instant.  C: how the caller keeps the count -- double as the planes do, or an integer that converts to the same
// double (the bulk kernel's registers).
template <class C>
K2R_HD K2R_FP_STRICT_FN void moment_step(C& c, double& K, double& s1, double& s2, double x) {
    K2R_FP_STRICT
    const bool ok = x == x;
    K = ok && c == (C)0 ? x : K;
    const double d = x - K;
    const double p = d * d;
    const double a1 = s1 + d, a2 = s2 + p;
    s1 = ok ? a1 : s1;
    s2 = ok ? a2 : s2;
    c = ok ? c + (C)1 : c;
}
K2R_HD void moment_step(MomentState& s, double x) { moment_step(s.c, s.K, s.s1, s.s2, x); }

// sqrt of a finite v > 0, correctly rounded whatever the platform's sqrt returns within an ulp: Tuckerman's test of the
// candidate against its two neighbours, s is the rounded root exactly when s * pred(s) < v <= s * succ(s); the residuals' signs
// come from one fma each.  (Where sqrt is IEEE's -- every host -- neither branch is ever taken.)  Below 2^-900 a residual could
// round to zero; no raster reaches that -- a leaf's non-zero |d| is at least 2^-63 -- and the candidate is returned as it is.
K2R_HD double moment_sqrt(double v) {
    const double s = sqrt(v);
    if (!(v >= 0x1p-900) || !(v < __builtin_inf())) return s;
    uint64_t b;
    __builtin_memcpy(&b, &s, 8);
    const uint64_t bd = b - 1u, bu = b + 1u;
    double dn, up;
    __builtin_memcpy(&dn, &bd, 8);
    __builtin_memcpy(&up, &bu, 8);
    if (__builtin_fma(s, dn, -v) >= 0.0) return dn;
    if (__builtin_fma(s, up, -v) < 0.0) return up;
    return s;
}

// A state into (COUNT, MEAN, VAR, STD).  ddof: 0 or 1.
K2R_HD K2R_FP_STRICT_FN void moment_finish(const MomentState& s, uint32_t ddof, double (&out)[4]) {
    K2R_FP_STRICT
    // (every NaN below is written as the one quiet NaN, not as what 0 / 0 leaves on the platform)
    const double m = s.s1 / s.c;
    out[0] = s.c;
    out[1] = s.c > 0.0 ? s.K + m : __builtin_nan("");
    const double p = s.s1 * m;
    double q = s.s2 - p;
    if (q < 0.0) q = 0.0;
    out[2] = s.c > (double)ddof ? q / (s.c - (double)ddof) : __builtin_nan("");
    out[3] = s.c > (double)ddof ? moment_sqrt(out[2]) : __builtin_nan("");
}

// ---- per cell, a run of equal labels at a time: what the fold kernel's MomentCell and the host check run ------------------------
// instant i's label; without a label array every instant is group 0
K2R_HD uint32_t moment_label(const uint16_t* labels, uint64_t i) { return labels ? (uint32_t)labels[i] : 0u; }
// The four state planes of one cell: element (group 0, the cell); group g is g * gsz on.
struct MomentPlanes {
    double *p_c, *p_k, *p_s1, *p_s2;
    uint64_t gsz;
};
K2R_HD MomentPlanes moment_planes(double* dst, double* scr, uint32_t ops, uint64_t o_off, uint64_t s_off, uint64_t psz, uint64_t gsz) {
    return MomentPlanes{moment_plane(MS_COUNT, dst, scr, ops, o_off, s_off, psz), moment_plane(MS_K, dst, scr, ops, o_off, s_off, psz),
                        moment_plane(MS_S1, dst, scr, ops, o_off, s_off, psz), moment_plane(MS_S2, dst, scr, ops, o_off, s_off, psz), gsz};
}
// the state of the open run of group g (GROUP_NONE: no run is open)
struct MomentRun {
    MomentState s;
    uint32_t g;
};
K2R_HD MomentRun moment_run_init() { return MomentRun{moment_init(), GROUP_NONE}; }
// the open run's state into its group's planes, whole
K2R_HD void moment_store(const MomentRun& st, const MomentPlanes& P) {
    if (st.g == GROUP_NONE) return;
    const uint64_t at = (uint64_t)st.g * P.gsz;
    P.p_c[at] = st.s.c;
    P.p_k[at] = st.s.K;
    P.p_s1[at] = st.s.s1;
    P.p_s2[at] = st.s.s2;
}
// One instant with label `label` and value x into the run.  On a change of group the old group's state is stored and the new
// group's loaded; an instant of no group changes nothing.
K2R_HD void moment_group_step(MomentRun& st, const MomentPlanes& P, uint32_t label, uint32_t n_groups, double x) {
    if (label >= n_groups) return;
    if (label != st.g) {
        moment_store(st, P);
        const uint64_t at = (uint64_t)label * P.gsz;
        st.g = label;
        st.s = MomentState{P.p_c[at], P.p_k[at], P.p_s1[at], P.p_s2[at]};
    }
    moment_step(st.s, x);
}

#if defined(__HIPCC__)
struct ChunkRef;
// k_bulk_moment over n units on the null stream (asynchronous).  d_enc: the chunks' encodings; d_labels: the call's labels, or
// nullptr (every instant is group 0).  Returns a DCDF code.
int launch_bulk_moment(const ChunkRef* d_refs, const uint8_t* d_enc, const GroupUnit* d_units, uint32_t n, const uint16_t* d_labels,
                       uint32_t n_groups, double* d_dst, double* d_scr, uint32_t ops);
#endif

}  // namespace k2r
