// k2r_regress.h -- regression over time, the contract: the per-cell state, its step and its finish, as dcdf_regress_host
// (k2r_raster_region.hip) runs them on the host.  Compiles for the host alone as well (g++).  No kernel runs them yet: the raster
// entry points are not built.
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

}  // namespace k2r
