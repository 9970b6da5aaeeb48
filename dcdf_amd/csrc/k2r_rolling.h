// k2r_rolling.h -- rolling windows over time: per cell, the extremes of the sums (or means) of every w consecutive instants, when
// they occurred and how many windows counted -- the per-cell state, its steps and its finish, and the cell body that walks one
// cell's series through them (rolling_cell): what the planner (plan_rolling_time, k2r_plan.h), the stream kernel
// (k_rolling_stream, k2r_rolling.hip) and the host checks (tests/sim) share.  Compiles for the host alone as well (g++).
// DESIGN.md section 4o.
//
// The contract (include/dcdf_k2r.h): x[i] is reduce_widen of the cell's stored integer at instant i, counted
// from the cube's first.  The window that ENDS at instant i covers [i - w + 1, i] and exists for i >= w - 1; c_i is the number of
// its non-NaN values, S_i their exact real sum; it is valid iff c_i >= min_count.  MAX / MIN: the greatest / least S_i over the
// valid windows, rounded ONCE to the nearest double, ties to even (space_round; a sum of 0 is +0.0), for the mean divided by
// (double)w, one IEEE division (min_count == w then: every valid window has w values).  ARGMAX / ARGMIN: the least i whose exact
// S_i is the greatest / least -- compared as integers, so two sums that round to one double are no tie.  COUNT: the valid
// windows.  None: NaN, NaN, NaN, NaN, +0.0.  In the grouped call a window belongs to the group of its LAST instant and reaches
// back over instants of any label or none.
//
// Why it is exact: every non-NaN x is (-1)^sign * m * 2^shift / 2^63 with an integer m (k2r_space.h), so a window's sum at the
// 2^-63 scale is a 192-bit integer (65535 values below 2^127 each stay below 2^143).  Integers add and subtract exactly:
// SLIDING a window (add the entering value, subtract the leaving one) and RE-SUMMING it leave the same 192 bits, and the
// result depends on no cut of the work, no order and no choice between the two.
#pragma once
#include "k2r_quantile.h"
#include "k2r_space.h"

namespace k2r {

// the statistics (DCDF_ROLLING_*), in plane order; the kinds
constexpr uint32_t RW_MAX = 1u, RW_ARGMAX = 2u, RW_MIN = 4u, RW_ARGMIN = 8u, RW_COUNT = 16u, RW_ALL = 31u;
constexpr int32_t ROLLING_SUM = 0, ROLLING_MEAN = 1;
constexpr uint32_t ROLLING_MAX_WINDOW = 65535u;

// the call's own arguments: a set of statistics, 1 <= min_count <= window <= 65535, a kind; a mean over a varying count is not an
// order on the sums, so MEAN takes whole windows only
K2R_HD bool rolling_args_ok(uint32_t ops, uint32_t window, uint32_t min_count, int32_t kind) {
    return ops != 0 && ops <= RW_ALL && window >= 1u && window <= ROLLING_MAX_WINDOW && min_count >= 1u && min_count <= window &&
           (kind == ROLLING_SUM || (kind == ROLLING_MEAN && min_count == window));
}

// ---- one value at the 2^-63 scale ---------------------------------------------------------------------------------------------------
// x * 2^63 of the stored integer n of a leaf (enc, fbits) as a 192-bit two's complement integer; ok: x is not NaN (else 0 comes
// back).  space_m is the integer the decoder itself rounds to, so this is reduce_widen's x and no other.
K2R_HD U192 rolling_term(int32_t enc, uint32_t fbits, int64_t n, bool& ok) {
    ok = enc == ENC_I32 || enc == ENC_I64 || n != 0;
    const double d = space_m(enc, n);
    const uint32_t sc = space_scale(enc, fbits), sh = sc & 255u;
    const uint64_t mag = ok ? space_mag(d) : 0u;
    const U192 v{mag << sh, sh ? mag >> (64u - sh) : 0u, 0u};
    return (d < 0) != ((sc & SPACE_NEG) != 0) ? u192_neg(v) : v;
}
// a < b as signed 192-bit integers
K2R_HD bool u192_less(const U192& a, const U192& b) {
    if (a.w2 != b.w2) return (int64_t)a.w2 < (int64_t)b.w2;
    if (a.w1 != b.w1) return a.w1 < b.w1;
    return a.w0 < b.w0;
}

// ---- the state of one cell and group ------------------------------------------------------------------------------------------------
struct RollingState {
    U192 sum;      // of the non-NaN values of the window at hand
    uint32_t cnt;  // their number
    U192 mx, mn;   // the extreme sums of the valid windows so far (meaningless while valid == 0)
    uint32_t amx, amn, valid;
};
K2R_HD RollingState rolling_init() { return RollingState{U192{0, 0, 0}, 0u, U192{0, 0, 0}, U192{0, 0, 0}, 0u, 0u, 0u}; }
K2R_HD void rolling_clear(RollingState& s) {
    s.sum = U192{0, 0, 0};
    s.cnt = 0u;
}
// a value enters / leaves the window (a NaN changes nothing)
K2R_HD void rolling_add(RollingState& s, int32_t enc, uint32_t fbits, int64_t n) {
    bool ok;
    const U192 v = rolling_term(enc, fbits, n, ok);
    u192_add(s.sum, v);
    s.cnt += ok ? 1u : 0u;
}
K2R_HD void rolling_sub(RollingState& s, int32_t enc, uint32_t fbits, int64_t n) {
    bool ok;
    const U192 v = u192_neg(rolling_term(enc, fbits, n, ok));
    u192_add(s.sum, v);
    s.cnt -= ok ? 1u : 0u;
}
// the window that ends at instant t is complete: into the extremes when it is valid.  Instants come ascending, so a strict
// comparison keeps the least instant of equal sums.  Written with selects: a wave's lanes differ here.
K2R_HD void rolling_fold(RollingState& s, uint32_t t, uint32_t min_count) {
    const bool ok = s.cnt >= min_count, first = s.valid == 0u;
    const bool up = ok && (first || u192_less(s.mx, s.sum)), dn = ok && (first || u192_less(s.sum, s.mn));
    s.mx.w0 = up ? s.sum.w0 : s.mx.w0, s.mx.w1 = up ? s.sum.w1 : s.mx.w1, s.mx.w2 = up ? s.sum.w2 : s.mx.w2;
    s.mn.w0 = dn ? s.sum.w0 : s.mn.w0, s.mn.w1 = dn ? s.sum.w1 : s.mn.w1, s.mn.w2 = dn ? s.sum.w2 : s.mn.w2;
    s.amx = up ? t : s.amx;
    s.amn = dn ? t : s.amn;
    s.valid += ok ? 1u : 0u;
}
// A state into (MAX, ARGMAX, MIN, ARGMIN, COUNT).  The one rounding is space_round's; the mean's division is one IEEE division.
K2R_HD void rolling_finish(const RollingState& s, uint32_t window, int32_t kind, double (&out)[5]) {
    const bool any = s.valid != 0u;
    double mx = space_round(s.mx), mn = space_round(s.mn);
    if (kind == ROLLING_MEAN) {
        const double w = (double)window;
        mx = mx / w;
        mn = mn / w;
    }
    out[0] = any ? mx : __builtin_nan("");
    out[1] = any ? (double)s.amx : __builtin_nan("");
    out[2] = any ? mn : __builtin_nan("");
    out[3] = any ? (double)s.amn : __builtin_nan("");
    out[4] = (double)s.valid;
}

// ---- the column stream ---------------------------------------------------------------------------------------------------------
// The cube is decoded band by band into plan_quantile_time's slab of stored integers (k2r_plan.h), as for regress_time
// (k2r_regress.h); a lane per cell then reads its own series from there.  What a cell needs beside its column is the same for
// every cell of its cube:
//   seg_of    for EVERY instant of the cube the entry of the column's segment table that widens it (segments cut time only: the
//             index is the same in every column) -- a window's tail and a rebuilt window reach over instants of any label;
//   ends      the instants i >= w - 1 that belong to a group, sorted by (group, instant): the windows' last instants;
//   start     a CSR over them, start[g] .. start[g + 1] the windows of group g (the plain call: one group, every window).
struct RollingCol {
    QuantileCol q;
    uint32_t end0, start0, seg_of0, _pad;  // where its cube's ends, CSR and instant table begin
};
constexpr uint32_t ROLLING_AHEAD = 4;  // instants whose head and tail values are read before the first enters the carry chain

// One cell from end to end, as the kernel runs it.  read(t) is the cell's stored integer at instant t; put(i, v) takes element v
// of plane i = (place of the statistic among those of `ops`) * n_groups + g.  Per group the windows are walked in ascending
// order: the first of a run of consecutive instants is REBUILT from its w values, each further one SLIDES -- so the plain
// call and contiguous groups (years, months) rebuild once per run, a scattered labelling (i % 7) every window, O(w) reads
// each.  The reads of a batch depend on no state, so they are all issued before the batch's first addition.  Every plane gets
// its value exactly once: a group without a window finishes the initial state.
template <class Read, class Put>
K2R_HD void rolling_cell(const uint32_t* ends, const uint32_t* start, uint32_t n_groups, const uint32_t* seg_of, const QuantileSeg* segs,
                         uint32_t ops, uint32_t window, uint32_t min_count, int32_t kind, Read&& read, Put&& put) {
    for (uint32_t g = 0; g < n_groups; g++) {
        RollingState s = rolling_init();
        uint32_t j = start[g];
        const uint32_t j1 = start[g + 1u];
        while (j < j1) {
            uint32_t t = ends[j++];
            // rebuild: the w values of [t - w + 1, t]
            rolling_clear(s);
            uint32_t u = t + 1u - window;
            for (; t + 1u - u >= ROLLING_AHEAD; u += ROLLING_AHEAD) {
                int64_t n[ROLLING_AHEAD];
                QuantileSeg G[ROLLING_AHEAD];
#pragma unroll
                for (uint32_t k = 0; k < ROLLING_AHEAD; k++) n[k] = read(u + k);
#pragma unroll
                for (uint32_t k = 0; k < ROLLING_AHEAD; k++) G[k] = segs[seg_of[u + k]];
#pragma unroll
                for (uint32_t k = 0; k < ROLLING_AHEAD; k++) rolling_add(s, G[k].enc, G[k].fbits, n[k]);
            }
            for (; u <= t; u++) {
                const QuantileSeg G = segs[seg_of[u]];
                rolling_add(s, G.enc, G.fbits, read(u));
            }
            rolling_fold(s, t, min_count);
            // slide: the run of instants that follow t directly
            while (j < j1 && ends[j] == t + 1u) {
                if (j1 - j >= ROLLING_AHEAD && ends[j + ROLLING_AHEAD - 1u] == t + ROLLING_AHEAD) {  // (ascending: all four follow)
                    int64_t nh[ROLLING_AHEAD], nl[ROLLING_AHEAD];
                    QuantileSeg Gh[ROLLING_AHEAD], Gl[ROLLING_AHEAD];
#pragma unroll
                    for (uint32_t k = 0; k < ROLLING_AHEAD; k++) nh[k] = read(t + 1u + k);
#pragma unroll
                    for (uint32_t k = 0; k < ROLLING_AHEAD; k++) nl[k] = read(t + 1u + k - window);
#pragma unroll
                    for (uint32_t k = 0; k < ROLLING_AHEAD; k++) Gh[k] = segs[seg_of[t + 1u + k]], Gl[k] = segs[seg_of[t + 1u + k - window]];
#pragma unroll
                    for (uint32_t k = 0; k < ROLLING_AHEAD; k++) {
                        rolling_add(s, Gh[k].enc, Gh[k].fbits, nh[k]);
                        rolling_sub(s, Gl[k].enc, Gl[k].fbits, nl[k]);
                        rolling_fold(s, t + 1u + k, min_count);
                    }
                    t += ROLLING_AHEAD;
                    j += ROLLING_AHEAD;
                } else {
                    t++;
                    j++;
                    const QuantileSeg Gh = segs[seg_of[t]], Gl = segs[seg_of[t - window]];
                    const int64_t nh = read(t), nl = read(t - window);
                    rolling_add(s, Gh.enc, Gh.fbits, nh);
                    rolling_sub(s, Gl.enc, Gl.fbits, nl);
                    rolling_fold(s, t, min_count);
                }
            }
        }
        double o[5];
        rolling_finish(s, window, kind, o);
        uint32_t plane = g;
#pragma unroll
        for (uint32_t k = 0; k < 5u; k++)
            if (ops >> k & 1u) {
                put(plane, o[k]);
                plane += n_groups;
            }
    }
}

#if defined(__HIPCC__)
// k_rolling_stream over n columns on the null stream (asynchronous); max_cells: of the largest of them.  Returns a DCDF code.
int launch_rolling_stream(const RollingCol* d_cols, uint32_t n, uint64_t max_cells, const QuantileSeg* d_segs, const uint32_t* d_ends,
                          const uint32_t* d_start, const uint32_t* d_seg_of, uint32_t n_groups, const int64_t* d_slab, uint32_t ops,
                          uint32_t window, uint32_t min_count, int32_t kind, double* d_dst);
#endif

}  // namespace k2r
