// k2r_space.h -- reduction over space (dcdf_raster_reduce_space_batch): what the planner (k2r_plan.h), the bulk kernel
// (k2r_bulk.hip) and the fold / finish kernels share.  Everything here compiles for the host alone as well (g++), so the
// arithmetic the result rests on can be run and sanitised on a CPU.
//
// The contract (include/dcdf_k2r.h): per instant, over the selected cells of a cube, x = reduce_widen of
// the stored integer; MIN / MAX = fmin / fmax over the non-NaN x; COUNT = their number; SUM = their exact real sum rounded once
// to the nearest double (ties to even); MEAN = SUM / COUNT.
//
// Why the sum is exact: every non-NaN x of one leaf is s * m * 2^shift / 2^63 with an integer m, |m| <= 2^63, one shift in
// 0 .. 63 and one sign s per leaf (space_m, space_scale below), so a piece's sum is the INTEGER sum of its m -- associative, any
// order, any cut -- and the cube's sum is the 192-bit integer sum of the pieces' sums at the common 2^-63 scale, converted once.
#pragma once
#include "k2r_decode.h"

namespace k2r {

// ---- the value of one cell as an integer at its leaf's scale ---------------------------------------------------------------
// scale word of a leaf: bits 0..7 = shift, bit 8 = the sign is negative.  x * 2^63 = (-1)^sign * m * 2^shift.
// Integer leaves: x = m.  Float leaves: x = m / (+-2^(fbits + 1)) (from_fixed, k2r_decode.h); with 62 fractional bits the divisor
// (int64_t)1 << 63 is -2^63, the wrapped divisor value_bounds and reduce_fold4 know.
constexpr uint32_t SPACE_NEG = 256u;
K2R_HD uint32_t space_scale(int32_t enc, uint32_t fbits) {
    if (enc == ENC_I32 || enc == ENC_I64) return 63u;
    return (62u - fbits) | (fbits == 62u ? SPACE_NEG : 0u);
}
// m of the stored integer n (n != 0 for float leaves), as the integer-valued double the decoder itself forms before it
// divides: (double)n rounds beyond 2^53, (float)(n - 1) beyond 2^24 -- m is the ROUNDED integer, so that x is reduce_widen's
K2R_HD double space_m(int32_t enc, int64_t n) {
    switch (enc) {
        case ENC_I32: return (double)(int32_t)n;
        case ENC_I64: return (double)n;
        case ENC_F32: return (double)(float)(n - 1);
        default: return (double)(n - 1);
    }
}
// |d| of an integer-valued double, |d| <= 2^63, as an unsigned integer
K2R_HD uint64_t space_mag(double d) {
    const double a = d < 0 ? -d : d;
    return a >= 9223372036854775808.0 ? (uint64_t)1 << 63 : (uint64_t)a;
}
// (hi, lo) += d: a two's complement 128-bit sum of m's (up to 2^32 cells of |m| <= 2^63 fit)
K2R_HD void space_add_m(uint64_t& hi, uint64_t& lo, double d) {
    const uint64_t mag = space_mag(d);
    if (d < 0) {
        hi -= lo < mag ? 1u : 0u;
        lo -= mag;
    } else {
        const uint64_t l = lo + mag;
        hi += l < lo ? 1u : 0u;
        lo = l;
    }
}
K2R_HD void space_add128(uint64_t& hi, uint64_t& lo, uint64_t bhi, uint64_t blo) {
    const uint64_t l = lo + blo;
    hi += bhi + (l < lo ? 1u : 0u);
    lo = l;
}
// (hi, lo) = d * cnt: an elided piece, whose selected cells all hold one value
K2R_HD void space_mul_m(uint64_t& hi, uint64_t& lo, double d, uint32_t cnt) {
    const uint64_t mag = space_mag(d);
    const uint64_t p0 = (mag & 0xffffffffu) * cnt, p1 = (mag >> 32) * cnt;
    lo = p0 + (p1 << 32);
    hi = (p1 >> 32) + (lo < p0 ? 1u : 0u);
    if (d < 0) {
        lo = ~lo + 1u;
        hi = ~hi + (lo == 0 ? 1u : 0u);
    }
}

// ---- one record per (piece, instant) ----------------------------------------------------------------------------------------
// The statistics of one piece's selected cells at one instant: the 128-bit sum of m (two's complement), the count of non-NaN
// values, the extremes already widened (NaN: none), and the leaf's scale word.
struct SpacePartial {
    uint64_t hi, lo;
    double mn, mx;
    uint32_t cnt, scale;
};
static_assert(sizeof(SpacePartial) == 40, "the planner sizes the scratch by it");

// ---- 192-bit two's complement integers: the cube's sum at the 2^-63 scale ----------------------------------------------------
struct U192 {
    uint64_t w0, w1, w2;  // least significant first
};
K2R_HD void u192_add(U192& a, const U192& b) {
    const uint64_t s0 = a.w0 + b.w0, c0 = s0 < a.w0 ? 1u : 0u;
    const uint64_t s1 = a.w1 + b.w1, c1 = s1 < a.w1 ? 1u : 0u;
    const uint64_t t1 = s1 + c0, c2 = t1 < s1 ? 1u : 0u;
    a.w2 = a.w2 + b.w2 + c1 + c2;
    a.w1 = t1;
    a.w0 = s0;
}
K2R_HD U192 u192_neg(const U192& a) {
    U192 r{~a.w0 + 1u, ~a.w1, ~a.w2};
    if (r.w0 == 0) {
        r.w1 += 1u;
        if (r.w1 == 0) r.w2 += 1u;
    }
    return r;
}
// a record's sum at the common scale: sign-extended, shifted left by its shift, negated where its sign says so
K2R_HD U192 space_scaled(uint64_t hi, uint64_t lo, uint32_t scale) {
    const uint32_t sh = scale & 255u;
    const uint64_t ext = (hi >> 63) ? ~(uint64_t)0 : 0u;
    U192 r{lo, hi, ext};
    if (sh) {
        r.w0 = lo << sh;
        r.w1 = (hi << sh) | (lo >> (64u - sh));
        r.w2 = (ext << sh) | (hi >> (64u - sh));
    }
    return (scale & SPACE_NEG) ? u192_neg(r) : r;
}
// limb i of m (selects, not an indexed array: device code keeps it in registers)
K2R_HD uint64_t u192_limb(const U192& m, uint32_t i) { return i == 0 ? m.w0 : i == 1 ? m.w1 : i == 2 ? m.w2 : 0u; }
// the low 64 bits of m >> s
K2R_HD uint64_t u192_shr64(const U192& m, uint32_t s) {
    const uint32_t wi = s >> 6, b = s & 63u;
    const uint64_t a = u192_limb(m, wi), c = u192_limb(m, wi + 1u);
    return b ? (a >> b) | (c << (64u - b)) : a;
}
// any bit of m below bit k
K2R_HD bool u192_low_any(const U192& m, uint32_t k) {
    bool any = false;
    for (uint32_t i = 0; i < 3u; i++) {
        const uint64_t w = u192_limb(m, i);
        if (k >= 64u * (i + 1u)) any = any || w != 0;
        else if (k > 64u * i) any = any || (w & (((uint64_t)1 << (k - 64u * i)) - 1u)) != 0;
    }
    return any;
}
K2R_HD double space_pow2(int32_t k) {  // 2^k, -1022 <= k <= 1023
    const uint64_t bits = (uint64_t)(k + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return d;
}
// v / 2^63 as the nearest double, ties to even; +0.0 for 0.  |v| < 2^191, so the result is a normal number (or 0): one rounding.
K2R_HD double space_round(const U192& v) {
    const bool neg = (v.w2 >> 63) != 0;
    const U192 m = neg ? u192_neg(v) : v;
    if ((m.w0 | m.w1 | m.w2) == 0) return 0.0;
    const uint32_t p = m.w2 ? 191u - (uint32_t)__builtin_clzll(m.w2) : m.w1 ? 127u - (uint32_t)__builtin_clzll(m.w1) : 63u - (uint32_t)__builtin_clzll(m.w0);
    uint64_t q = m.w0;
    uint32_t s = 0;
    if (p > 52u) {  // keep the 53 bits from p down; round on the bit below them and the rest
        s = p - 52u;
        q = u192_shr64(m, s);
        const bool half = (u192_shr64(m, s - 1u) & 1u) != 0;
        if (half && (u192_low_any(m, s - 1u) || (q & 1u))) q += 1u;  // (q may become 2^53: still exact as a double)
    }
    const double r = (double)q * space_pow2((int32_t)s - 63);
    return neg ? -r : r;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// One workgroup's work in k_bulk_space: BulkUnit (k2r_bulk.h) with the place of its records and of its cells' mask bytes instead
// of the output strides.  The record of instant t is recs[rec + (t - t0)].
struct SpaceUnit {
    uint32_t chunk;  // index into the ChunkRef table
    uint32_t t0, t1;
    uint16_t rr, rc;
    uint16_t top, bottom, left, right;
    uint32_t m_sr;   // row stride of the mask in bytes (the cube's columns)
    uint64_t rec;
    uint64_t m_off;  // mask byte of cell (top, left)
};
// A fallback or elided piece folded by k_space_fold.  src: element of (first instant, first row, first column) in the slab of
// stored integers, dense [nt][rows][cols]; for an elided piece the index of its first instant in dcdf_raster::d_vals.  The
// record of the piece's instant i is recs[rec + i].
struct SpaceFold {
    uint32_t nt, rows, cols, m_sr;
    int32_t enc;
    uint32_t fbits, elided, _pad;
    uint64_t src, rec, m_off;
};
// What k_space_finish folds into nt results of one cube: the records recs[rec + slot * nt + i], slot < n_slots, of instant i;
// statistic k of the cube (in ascending bit order) goes to dst[o_off + k * o_stride + i].
struct SpaceJob {
    uint64_t rec;
    uint32_t n_slots, nt;
    uint64_t o_off, o_stride;
};

#if defined(__HIPCC__)
struct ChunkRef;
// k_bulk_space over n units on the null stream (asynchronous).  d_enc: the chunks' encodings; d_mask: the masks' bytes or null;
// live: the accumulators the statistics need (reduce_live, k2r_reduce.h).  Returns a DCDF code.
int launch_bulk_space(const ChunkRef* d_refs, const uint8_t* d_enc, const SpaceUnit* d_units, uint32_t n, const uint8_t* d_mask,
                      SpacePartial* d_recs, uint32_t live);
#endif

}  // namespace k2r
