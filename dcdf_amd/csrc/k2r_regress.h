// k2r_regress.h -- regression over time: the per-cell state, its step and its finish, and the cell body that streams one cell's
// series through them (regress_cell) -- what dcdf_regress_host (k2r_raster_region.hip), the planner (plan_regress_time,
// k2r_plan.h), the stream kernel (k_regress_stream, k2r_regress.hip) and the host checks (tests/sim) share.  Compiles for the host
// alone as well (g++).  DESIGN.md section 4n.
//
// The contract (include/dcdf_k2r.h): the least-squares line of a series x[t] against a per-instant regressor
// e[t].  The state is seven doubles (c, K, sy, syy, se, see, sey), at first (0, NaN, +0.0, +0.0, +0.0, +0.0, +0.0).  In instant
// order every instant t with a non-NaN x[t] does
//     if (c == 0) K = x;  d = x - K;
//     sy = sy + d;  syy = syy + d * d;  se = se + e;  see = see + e * e;  sey = sey + e * d;  c = c + 1
// -- each one IEEE double operation, nothing contracted into an fma (regress_step); a NaN x changes nothing.  K, the shift of
// the values, is the series' first value as in the moments (k2r_moment.h).  The regressor enters exactly as given -- nothing
// shifts it here --, so the sums see, sey keep their accuracy only for a regressor near zero: |e| of the order of its own
// spread.  A caller with a far-off regressor (years, time stamps) subtracts its first value before the call.  Finishing
// (regress_finish): n = c, me = se / n, my = sy / n, See = max(see - se * me, +0.0), Syy = max(syy - sy * my, +0.0), Sey = sey -
// se * my; COUNT = c; SLOPE = Sey / See when c >= 2 and See > 0, else NaN; INTERCEPT = (K + my) - SLOPE * me -- the fitted value at
// e = 0 --, NaN when SLOPE is; CORR = Sey / sqrt(See * Syy) (the root correctly rounded, moment_sqrt) clamped to [-1, 1] when
// additionally Syy > 0, else NaN.  Every NaN is the one quiet NaN.  Consequences: a constant series has SLOPE exactly +0.0,
// INTERCEPT its value and CORR NaN; one valid instant gives NaN but for COUNT; for integer values with |x| < 2^53 a constant added
// to every value changes no bit of SLOPE or CORR (every d is exact).  The state is loaded and stored whole -- there is no merge
// rule --, so the result depends on no cut of a series' instants.
#pragma once
#include "k2r_moment.h"
#include "k2r_quantile.h"

namespace k2r {

// the statistics (DCDF_REGRESS_*), in plane order
constexpr uint32_t RO_COUNT = 1u, RO_SLOPE = 2u, RO_INTERCEPT = 4u, RO_CORR = 8u, RO_ALL = 15u;

struct RegressState {
    double c, K, sy, syy, se, see, sey;
};
K2R_HD RegressState regress_init() { return RegressState{0.0, __builtin_nan(""), 0.0, 0.0, 0.0, 0.0, 0.0}; }

// whether a regressor value is finite, read from its exponent bits (no floating-point operation: no compiler flag changes it)
K2R_HD bool regress_finite(double e) {
    uint64_t b;
    __builtin_memcpy(&b, &e, 8);
    return ((b >> 52) & 0x7ffu) != 0x7ffu;
}

// One value x with its instant's regressor value e into a state; a NaN x changes nothing.  Written with selects as moment_step is.
K2R_HD K2R_FP_STRICT_FN void regress_step(RegressState& s, double x, double e) {
    K2R_FP_STRICT
    const bool ok = x == x;
    s.K = ok && s.c == 0.0 ? x : s.K;
    const double d = x - s.K;
    const double pd = d * d, pe = e * e, ped = e * d;
    const double a1 = s.sy + d, a2 = s.syy + pd, a3 = s.se + e, a4 = s.see + pe, a5 = s.sey + ped;
    s.sy = ok ? a1 : s.sy;
    s.syy = ok ? a2 : s.syy;
    s.se = ok ? a3 : s.se;
    s.see = ok ? a4 : s.see;
    s.sey = ok ? a5 : s.sey;
    s.c = ok ? s.c + 1.0 : s.c;
}

// A state into (COUNT, SLOPE, INTERCEPT, CORR).
K2R_HD K2R_FP_STRICT_FN void regress_finish(const RegressState& s, double (&out)[4]) {
    K2R_FP_STRICT
    // (every NaN below is written as the one quiet NaN, not as what 0 / 0 leaves on the platform)
    const double me = s.se / s.c, my = s.sy / s.c;
    const double pe = s.se * me, py = s.sy * my, pc = s.se * my;
    double See = s.see - pe, Syy = s.syy - py;
    const double Sey = s.sey - pc;
    if (See < 0.0) See = 0.0;
    if (Syy < 0.0) Syy = 0.0;
    const bool fit = s.c >= 2.0 && See > 0.0;
    const double slope = Sey / See;
    const double at0 = s.K + my, lift = slope * me;
    out[0] = s.c;
    out[1] = fit ? slope : __builtin_nan("");
    out[2] = fit ? at0 - lift : __builtin_nan("");
    out[3] = __builtin_nan("");
    if (fit && Syy > 0.0) {
        const double p = See * Syy;
        double r = Sey / moment_sqrt(p);
        if (r > 1.0) r = 1.0;
        if (r < -1.0) r = -1.0;
        out[3] = r;
    }
    for (int i = 1; i < 4; i++)  // (what an overflowed sum leaves: inf - inf)
        if (out[i] != out[i]) out[i] = __builtin_nan("");
}

// ---- the column stream ---------------------------------------------------------------------------------------------------------
// The raster calls decode a cube band by band into plan_quantile_time's slab of stored integers (k2r_plan.h); a lane per cell
// then reads its own series from there, once.  What a cell needs beside its column is the same for every cell of its cube:
//   records   one RegressRec per instant that belongs to a group, sorted by (group, instant): t, the instant counted from the
//             cube's first; seg, the entry of the column's segment table that widens it (segments cut time only: the index is the
//             same in every column of the cube); e, the cube's regressor value there;
//   start     a CSR over them, start[g] .. start[g + 1] the records of group g (the ungrouped call: one group, every instant).
struct RegressRec {
    double e;
    uint32_t t, seg;
};
static_assert(sizeof(RegressRec) == 16, "RegressRec");
// A column of the stream kernel: the selection kernel's, and where its cube's records and CSR begin
struct RegressCol {
    QuantileCol q;
    uint32_t rec0, start0;
};
constexpr uint32_t REGRESS_AHEAD = 4;  // slab values read before the first of them enters the chain of dependent additions

// One cell from end to end, as the kernel runs it: recs / start / segs are the cube's records, its CSR and the column's segment
// table; read(t) is the cell's stored integer at instant t, put(i, v) takes element v of plane i = (place of the statistic among
// those of `ops`) * n_groups + g.  Every plane gets its value exactly once: a group without a record finishes the initial state (0,
// NaN, NaN, NaN).  The reads of a batch depend on no state, so they are all issued before the batch's first step.
template <class Read, class Put>
K2R_HD void regress_cell(const RegressRec* recs, const uint32_t* start, uint32_t n_groups, const QuantileSeg* segs, uint32_t ops, Read&& read,
                         Put&& put) {
    for (uint32_t g = 0; g < n_groups; g++) {
        RegressState s = regress_init();
        uint32_t i = start[g];
        const uint32_t i1 = start[g + 1u];
        for (; i1 - i >= REGRESS_AHEAD; i += REGRESS_AHEAD) {
            RegressRec r[REGRESS_AHEAD];
            QuantileSeg G[REGRESS_AHEAD];
            int64_t n[REGRESS_AHEAD];
#pragma unroll
            for (uint32_t k = 0; k < REGRESS_AHEAD; k++) r[k] = recs[i + k];
#pragma unroll
            for (uint32_t k = 0; k < REGRESS_AHEAD; k++) n[k] = read(r[k].t);
#pragma unroll
            for (uint32_t k = 0; k < REGRESS_AHEAD; k++) G[k] = segs[r[k].seg];
#pragma unroll
            for (uint32_t k = 0; k < REGRESS_AHEAD; k++) regress_step(s, reduce_widen(G[k].enc, G[k].fbits, n[k]), r[k].e);
        }
        for (; i < i1; i++) {
            const QuantileSeg G = segs[recs[i].seg];
            regress_step(s, reduce_widen(G.enc, G.fbits, read(recs[i].t)), recs[i].e);
        }
        double o[4];
        regress_finish(s, o);
        uint32_t plane = g;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            if (ops >> k & 1u) {
                put(plane, o[k]);
                plane += n_groups;
            }
    }
}

#if defined(__HIPCC__)
// k_regress_stream over n columns on the null stream (asynchronous); max_cells: of the largest of them.  Returns a DCDF code.
int launch_regress_stream(const RegressCol* d_cols, uint32_t n, uint64_t max_cells, const QuantileSeg* d_segs, const RegressRec* d_recs,
                          const uint32_t* d_start, uint32_t n_groups, const int64_t* d_slab, uint32_t ops, double* d_dst);
#endif

}  // namespace k2r
