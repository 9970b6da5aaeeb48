// k2r_quantile.h -- per-cell quantiles over time (dcdf_raster_quantile_time_batch): what the planner (k2r_plan.h), the selection
// kernel (k2r_quantile.hip) and the host check (tests/sim/quantile_check.cpp) share.  Plain C++: compiles for the host alone (g++).
//
// The contract (include/dcdf_k2r.h): per cell, v[0 .. n) = the non-NaN x[t] of reduce_time in ascending
// order (-0.0 before +0.0); h = (double)(n - 1) * p, j = floor(h), g = h - j, j1 = min(j + 1, n - 1); the method picks v[j],
// v[j1] or v[j] + (v[j1] - v[j]) * g.  The result is exact: an order statistic is selected, never approximated.
//
// Selection works on order-preserving 64-bit keys of the doubles.  One pass over a cell's values gives, for the negative and for
// the other keys apart, their number and their AND and OR: within a sign the bits above the highest and below the lowest bit in
// which the keys differ are common to every key and are never looked at again (apart, since a negative double's trailing zeros
// are trailing ones of its key), and a target rank knows its sign from the two counts.  The bits between are consumed most
// significant first, QUANTILE_DIGIT at a time: a pass counts, for an interval of keys that share a prefix, the keys below each
// pivot of the next digit, and every target rank inside the interval moves into the sub-interval that holds it.  Target ranks
// that share their interval share its counters, so the probabilities of one call cost the passes of the distinct intervals they
// fall into, not one selection each; a pass takes the first G distinct unresolved intervals.  Everything is kept in registers:
// every loop over targets, groups and pivots has a compile-time bound and unrolls.
#pragma once
#include "k2r_reduce.h"

namespace k2r {

constexpr uint32_t QUANTILE_MAX_PROBS = 16;  // 1 <= n_probs <= 16: at most 32 target ranks (j and j1 of each)
enum : int32_t { QM_LOWER = 0, QM_HIGHER = 1, QM_NEAREST = 2, QM_LINEAR = 3 };  // DCDF_QUANTILE_*
constexpr uint32_t QUANTILE_DIGIT = 3;   // bits a pass consumes: 7 compare-adds per key and group
constexpr uint32_t QUANTILE_PIVOTS = (1u << QUANTILE_DIGIT) - 1u;
// G, the intervals a pass counts for: 2 for one probability (its j and j1 part early and then descend side by side), else 4
constexpr uint32_t quantile_groups(uint32_t R) { return R <= 2u ? 2u : 4u; }

inline bool quantile_args_ok(const double* probs, uint32_t n_probs, int32_t method) {
    if (!probs || n_probs < 1 || n_probs > QUANTILE_MAX_PROBS || method < QM_LOWER || method > QM_LINEAR) return false;
    for (uint32_t i = 0; i < n_probs; i++)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return false;  // (a NaN fails both)
    return true;
}

// ---- keys ----------------------------------------------------------------------------------------------------------------------
// The order-preserving key of a double that is not NaN (the caller skips NaN): unsigned compare of keys = numeric compare of the
// doubles, with -0.0 below +0.0.
K2R_HD uint64_t quantile_key(double d) {
    uint64_t b;
    __builtin_memcpy(&b, &d, sizeof b);
    return (b >> 63) ? ~b : b | ((uint64_t)1 << 63);
}
K2R_HD double quantile_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? k & ~((uint64_t)1 << 63) : ~k;
    double d;
    __builtin_memcpy(&d, &b, sizeof d);
    return d;
}

// ---- ranks -----------------------------------------------------------------------------------------------------------------------
// need: bit 0 = the method reads v[j], bit 1 = v[j1]
struct QuantileRank {
    uint32_t j, j1, need;
    double g;
};
K2R_HD QuantileRank quantile_rank(uint32_t n, double p, int32_t method) {  // n >= 1
    const double h = (double)(n - 1u) * p;  // one IEEE multiplication
    const double fl = __builtin_floor(h);
    QuantileRank r;
    r.j = (uint32_t)fl;
    r.g = h - fl;
    r.j1 = r.j + 1u < n ? r.j + 1u : n - 1u;
    switch (method) {
        case QM_LOWER: r.need = 1u; break;
        case QM_HIGHER: r.need = r.g == 0.0 ? 1u : 2u; break;
        case QM_NEAREST: r.need = r.g < 0.5 ? 1u : r.g > 0.5 ? 2u : (r.j & 1u) == 0u ? 1u : 2u; break;  // (at 0.5: the even one of j, j1)
        default: r.need = r.g == 0.0 ? 1u : 3u; break;
    }
    return r;
}
// LINEAR: three separate IEEE operations -- every unit that includes this is built without contraction (-ffp-contract=off)
K2R_HD double quantile_finish(const QuantileRank& r, double vj, double vj1) {
    if (r.need == 1u) return vj;
    if (r.need == 2u) return vj1;
    const double d = vj1 - vj;
    const double m = d * r.g;
    return vj + m;
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
K2R_HD uint32_t quantile_clz64(uint64_t x) { return (uint32_t)__builtin_clzll(x); }  // x != 0
K2R_HD uint32_t quantile_ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }

// The state of one cell: R target ranks, each with the interval [lo, lo + 2^sh) of keys (lo carries the bits common to the keys of
// its sign) that holds it and its rank `rel` among the keys of that interval.  A target is resolved when sh <= the lowest
// differing bit of its sign (lb[1] for keys with the top bit set, lb[0] for the negative ones): the interval then holds equal
// keys, lo itself.
template <uint32_t R>
struct QuantileCell {
    uint64_t lo[R];
    uint32_t rel[R], sh[R];
    uint32_t lb[2], n;
    K2R_HD uint32_t lb_of(uint64_t key) const { return (key >> 63) ? lb[1] : lb[0]; }
    K2R_HD bool unresolved() const {
        bool u = false;
#pragma unroll
        for (uint32_t k = 0; k < R; k++) u = u || sh[k] > lb_of(lo[k]);
        return u;
    }
};
// what one pass counts: for group i the keys of [glo, glo + 2^gsh) whose next digit (the bits [nsh, gsh)) is below pivot 1 .. 7
template <uint32_t G>
struct QuantilePass {
    uint64_t glo[G];
    uint32_t gsh[G], nsh[G], live[G];
    uint32_t c[G][QUANTILE_PIVOTS];
};
// what the first pass gathers of the keys of one sign
struct QuantileSign {
    uint32_t n;
    uint64_t a, o;  // AND and OR
};
K2R_HD void quantile_first_key(QuantileSign (&F)[2], uint64_t key) {
    const bool pos = (key >> 63) != 0u;
    F[0].n += pos ? 0u : 1u;
    F[1].n += pos ? 1u : 0u;
    F[0].a &= pos ? ~(uint64_t)0 : key;
    F[1].a &= pos ? key : ~(uint64_t)0;
    F[0].o |= pos ? (uint64_t)0 : key;
    F[1].o |= pos ? key : (uint64_t)0;
}

// after the first pass; n_probs probabilities of `method`: targets 2 i and 2 i + 1 are j and j1 of probs[i]
template <uint32_t R>
K2R_HD void quantile_begin(QuantileCell<R>& S, const QuantileSign (&F)[2], const double* probs, uint32_t n_probs, int32_t method) {
    uint64_t base[2];
    uint32_t top[2];
#pragma unroll
    for (uint32_t c = 0; c < 2u; c++) {
        const uint64_t diff = F[c].a ^ F[c].o;
        const bool flat = F[c].n == 0u || diff == 0u;  // nothing to select from, or one value: resolved at once
        top[c] = flat ? 0u : 64u - quantile_clz64(diff);  // the bits [lb, top) differ somewhere; top <= 63: the sign is common
        S.lb[c] = flat ? 0u : quantile_ctz64(diff);
        // the common bits: those from top on and those below lb
        const uint64_t low = ((uint64_t)1 << S.lb[c]) - 1u, high = ~(((uint64_t)1 << (top[c] & 63u)) - 1u);
        base[c] = flat ? F[c].a : F[c].a & (high | low);
    }
    const uint32_t n = F[0].n + F[1].n;
    S.n = n;
#pragma unroll
    for (uint32_t i = 0; i < R / 2u; i++) {
        QuantileRank r{0u, 0u, 1u, 0.0};
        if (i < n_probs && n != 0u) r = quantile_rank(n, probs[i], method);
#pragma unroll
        for (uint32_t e = 0; e < 2u; e++) {
            // (a rank the method does not read follows the one it reads)
            const uint32_t rank = e == 0u ? ((r.need & 1u) ? r.j : r.j1) : ((r.need & 2u) ? r.j1 : r.j);
            const uint32_t c = rank < F[0].n ? 0u : 1u;  // the negative keys come first
            S.lo[2u * i + e] = base[c];
            S.sh[2u * i + e] = i < n_probs ? top[c] : 0u;  // (a target beyond the call's probabilities: resolved)
            S.rel[2u * i + e] = rank - (c ? F[0].n : 0u);
        }
    }
}
// the groups of the next pass: the first G distinct intervals among the unresolved targets
template <uint32_t R, uint32_t G>
K2R_HD void quantile_pass_begin(const QuantileCell<R>& S, QuantilePass<G>& Q) {
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
        Q.live[i] = 0u;
        Q.glo[i] = 0u;
        Q.gsh[i] = 1u;
#pragma unroll
        for (uint32_t k = 0; k < R; k++) {
            bool fresh = Q.live[i] == 0u && S.sh[k] > S.lb_of(S.lo[k]);
#pragma unroll
            for (uint32_t e = 0; e < i; e++) fresh = fresh && !(Q.live[e] != 0u && Q.glo[e] == S.lo[k] && Q.gsh[e] == S.sh[k]);
            if (fresh) {
                Q.live[i] = 1u;
                Q.glo[i] = S.lo[k];
                Q.gsh[i] = S.sh[k];
            }
        }
        const uint32_t lb = S.lb_of(Q.glo[i]);
        const uint32_t left = Q.gsh[i] > lb ? Q.gsh[i] - lb : 1u;  // bits still to consume (a dead group: any)
        Q.nsh[i] = Q.gsh[i] - (left < QUANTILE_DIGIT ? left : QUANTILE_DIGIT);
#pragma unroll
        for (uint32_t d = 0; d < QUANTILE_PIVOTS; d++) Q.c[i][d] = 0u;
    }
}
template <uint32_t G>
K2R_HD void quantile_pass_key(QuantilePass<G>& Q, uint64_t key) {
#pragma unroll
    for (uint32_t i = 0; i < G; i++) {
        const bool in = Q.live[i] != 0u && ((key ^ Q.glo[i]) >> Q.gsh[i]) == 0u;  // (gsh <= 63)
        const uint32_t digit = in ? (uint32_t)(key >> Q.nsh[i]) & QUANTILE_PIVOTS : QUANTILE_PIVOTS;
#pragma unroll
        for (uint32_t d = 0; d < QUANTILE_PIVOTS; d++) Q.c[i][d] += digit < d + 1u ? 1u : 0u;
    }
}
// every target of a counted group moves into the sub-interval that holds its rank
template <uint32_t R, uint32_t G>
K2R_HD void quantile_pass_end(QuantileCell<R>& S, const QuantilePass<G>& Q) {
#pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        const uint64_t lo = S.lo[k];  // (two groups are never the same interval: at most one matches)
        const uint32_t sh = S.sh[k], lb = S.lb_of(lo);
#pragma unroll
        for (uint32_t i = 0; i < G; i++) {
            const bool mine = Q.live[i] != 0u && sh > lb && lo == Q.glo[i] && sh == Q.gsh[i];
            uint32_t digit = 0u, below = 0u;
#pragma unroll
            for (uint32_t d = 0; d < QUANTILE_PIVOTS; d++) {  // (the counts ascend with the pivot)
                const bool le = Q.c[i][d] <= S.rel[k];
                digit = le ? d + 1u : digit;
                below = le ? Q.c[i][d] : below;
            }
            if (mine) {
                S.lo[k] = lo | ((uint64_t)digit << Q.nsh[i]);
                S.rel[k] -= below;
                S.sh[k] = Q.nsh[i];
            }
        }
    }
}
// probability i of the call, once every target is resolved
template <uint32_t R>
K2R_HD double quantile_result(const QuantileCell<R>& S, uint32_t i, double p, int32_t method) {
    if (S.n == 0u) return __builtin_nan("");
    double vj = 0.0, vj1 = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < R / 2u; k++)
        if (k == i) {
            vj = quantile_unkey(S.lo[2u * k]);
            vj1 = quantile_unkey(S.lo[2u * k + 1u]);
        }
    return quantile_finish(quantile_rank(S.n, p, method), vj, vj1);
}
// One cell from end to end, as the kernel runs it: each(f) calls f(x) for every x[t] of the cell, any number of times over;
// any(b) is true while some cell that shares the pass loop is unresolved (a wave's lanes; the host: b itself); put(i, value)
// takes the result of probability i.  Returns the cell's own passes.
template <uint32_t R, class Each, class Any, class Put>
K2R_HD uint32_t quantile_cell(Each&& each, Any&& any, Put&& put, const double* probs, uint32_t n_probs, int32_t method) {
    QuantileSign F[2] = {{0u, ~(uint64_t)0, 0u}, {0u, ~(uint64_t)0, 0u}};
    each([&](double x) {
        if (x == x) quantile_first_key(F, quantile_key(x));
    });
    QuantileCell<R> S;
    quantile_begin(S, F, probs, n_probs, method);
    uint32_t passes = 0u;  // of this cell: those it was unresolved in
    for (;;) {
        const bool u = S.unresolved();
        if (!any(u)) break;
        passes += u ? 1u : 0u;
        QuantilePass<quantile_groups(R)> Q;
        quantile_pass_begin(S, Q);
        each([&](double x) {
            if (x == x) quantile_pass_key(Q, quantile_key(x));
        });
        quantile_pass_end(S, Q);
    }
#pragma unroll
    for (uint32_t i = 0; i < R / 2u; i++)
        if (i < n_probs) put(i, quantile_result(S, i, probs[i], method));
    return passes;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// A column of the selection kernel: the cells of one cube inside one leaf's place (cut further on the raster's 64-grid when its
// slab would be too large), over all the cube's instants.  Its stored integers lie in the band's slab, dense [nt][rows][cols]
// from element src; segment s of its table (segs[seg0 + s]) says how the instants from its t0 to the next entry's are widened.
// Plane i of the cube takes cell (r, c) at dst[o_off + i * psz + r * sr + c].
struct QuantileSeg {
    uint32_t t0;  // first instant, counted from the cube's
    int32_t enc;
    uint32_t fbits;
};
struct QuantileCol {
    uint32_t nt, rows, cols, sr;
    uint32_t seg0, nseg;
    uint64_t src, o_off, psz;
};
struct QuantileProbs {
    double p[QUANTILE_MAX_PROBS];
};

#if defined(__HIPCC__)
// k_quantile_select over n columns on the null stream (asynchronous); max_cells: of the largest of them.  Returns a DCDF code.
int launch_quantile_select(const QuantileCol* d_cols, uint32_t n, uint64_t max_cells, const QuantileSeg* d_segs, const int64_t* d_slab,
                           const QuantileProbs& probs, uint32_t n_probs, int32_t method, double* d_dst);
#endif

}  // namespace k2r
