// k2r_decode.h -- random access into encoded chunks: rank / DAC get / tree descent.
//
// Device-side restatement of the reference's query path over the SERIALIZED bytes (no pointer-rich
// in-memory structures): BitMap::get/rank (bitmap.rs:176-217), Dac::get (dac.rs:80-93),
// Snapshot::get/_search_window (snapshot.rs:165-188, 347-421), Log::get/_search_window
// (log.rs:176-293, 553-702).  The host parses the layout once (chunk.rs:247-266 et al.) into
// InstDesc records holding byte offsets; kernels then index the raw big-endian stream directly.
// Search is not in this header: its result SET is the reference's because decoding is exact and the one shape where the
// reference's own search is not "the cells in range" (log.rs:527-548) is carried as data (k2r_query.hip, SearchExtra).
#pragma once
#include "k2r_common.h"

namespace k2r {

struct BmDesc {  // bitmap.rs:128-138 as laid out in the stream
    uint32_t len;        // bits
    uint32_t k;          // index stride in words (4)
    uint32_t idx_off;    // byte offset of index[0]
    uint32_t words_off;  // byte offset of words[0]
};
struct DacDesc {  // dac.rs:37-44
    uint32_t nlev;
    BmDesc bm[8];
    uint32_t bytes_off[8];
};
struct InstDesc {  // one Snapshot (snapshot.rs:48-58) or Log (log.rs:53-64)
    uint32_t is_log;
    uint32_t snap;  // index of the owning block's snapshot InstDesc
    uint32_t k, rows, cols, sidelen;
    BmDesc T, E;
    DacDesc mx, mn;
};

K2R_HD uint32_t bmd_words(const BmDesc& d) { return (d.len + 31) / 32; }
K2R_HD bool bmd_get(const uint8_t* b, const BmDesc& d, uint32_t i) {  // bitmap.rs:176-183
    const uint32_t w = i >> 5;
    if (w >= bmd_words(d)) return false;  // the reference would panic; malformed input must not fault the GPU
    return (load_be32(b + d.words_off + 4 * w) >> (31 - (i & 31))) & 1u;
}
K2R_HD uint32_t bmd_rank(const uint8_t* b, const BmDesc& d, uint32_t i) {  // bitmap.rs:186-212
    if (i > d.len) i = d.len;
    const uint32_t block = (i >> 5) / d.k;
    uint32_t count = block > 0 ? load_be32(b + d.idx_off + 4 * (block - 1)) : 0;
    const uint32_t end = i >> 5;
    for (uint32_t w = block * d.k; w < end; w++) count += popc32(load_be32(b + d.words_off + 4 * w));
    const uint32_t left = i & 31;
    if (left) count += popc32(load_be32(b + d.words_off + 4 * end) >> (32 - left));
    return count;
}
K2R_HD uint32_t bmd_rank0(const uint8_t* b, const BmDesc& d, uint32_t i) { return i - bmd_rank(b, d, i); }

K2R_HD int64_t dacd_get(const uint8_t* b, const DacDesc& d, uint32_t index) {  // dac.rs:80-93
    uint64_t n = 0;
    for (uint32_t l = 0; l < d.nlev; l++) {
        if (index >= d.bm[l].len) break;  // malformed input guard
        n |= (uint64_t)b[d.bytes_off[l] + index] << (8 * l);
        if (bmd_get(b, d.bm[l], index)) index = bmd_rank(b, d.bm[l], index);
        else break;
    }
    return (int64_t)((n >> 1) ^ (0 - (n & 1)));  // zigzag_decode, dac.rs:139-142
}

// ---- point access --------------------------------------------------------------------------------
K2R_HD int64_t snapshot_get(const uint8_t* b, const InstDesc& S, uint32_t row, uint32_t col) {  // snapshot.rs:165-188
    int64_t max_value = dacd_get(b, S.mx, 0);
    if (!bmd_get(b, S.T, 0)) return max_value;
    const uint32_t k = S.k;
    uint32_t sl = S.sidelen, index = 0;
    for (int guard = 0; guard < 40 && sl > 1; guard++) {
        sl /= k;
        if (sl == 0) break;
        index = 1 + bmd_rank(b, S.T, index) * k * k + (row / sl) * k + col / sl;
        max_value -= dacd_get(b, S.mx, index);
        if (index >= S.T.len || !bmd_get(b, S.T, index)) return max_value;
        row %= sl;
        col %= sl;
    }
    return max_value;
}

K2R_HD int64_t log_get(const uint8_t* b, const InstDesc& S, const InstDesc& L, uint32_t row, uint32_t col) {
    // log.rs:176-293
    int64_t max_t = dacd_get(b, L.mx, 0);
    int64_t max_s = dacd_get(b, S.mx, 0);
    const bool single_t = !bmd_get(b, L.T, 0);
    const bool single_s = !bmd_get(b, S.T, 0);
    if (single_t && single_s) return max_t + max_s;
    if (single_t && !bmd_get(b, L.E, 0)) return max_t + max_s;
    bool has_t = !single_t, has_s = !single_s;
    uint32_t it = 0, is = 0;
    const uint32_t k = L.k;
    uint32_t sl = L.sidelen;
    for (int guard = 0; guard < 40 && sl > 1; guard++) {
        sl /= k;
        if (sl == 0) break;
        if (has_s) {
            is = 1 + bmd_rank(b, S.T, is) * k * k + (row / sl) * k + col / sl;
            max_s -= dacd_get(b, S.mx, is);
        }
        if (has_t) {
            it = 1 + bmd_rank(b, L.T, it) * k * k + (row / sl) * k + col / sl;
            max_t = dacd_get(b, L.mx, it);
        }
        // log.rs:240,245 write `>`; `>=` is identical wherever the reference does not panic
        const bool leaf_t = has_t ? (it >= L.T.len || !bmd_get(b, L.T, it)) : true;
        const bool leaf_s = has_s ? (is >= S.T.len || !bmd_get(b, S.T, is)) : true;
        if (leaf_t && leaf_s) return max_t + max_s;
        if (leaf_s) {
            has_s = false;
        } else if (leaf_t) {
            if (has_t && it < L.T.len) {
                const bool eq = bmd_get(b, L.E, bmd_rank0(b, L.T, it + 1) - 1);
                if (!eq) return max_t + max_s;
            }
            has_t = false;
        }
        row %= sl;
        col %= sl;
    }
    return max_t + max_s;
}

// value of (instant-desc i) at (row,col)
K2R_HD int64_t inst_get(const uint8_t* b, const InstDesc* descs, uint32_t i, uint32_t row, uint32_t col) {
    const InstDesc& D = descs[i];
    if (!D.is_log) return snapshot_get(b, D, row, col);  // block.rs:42-47
    return log_get(b, descs[D.snap], D, row, col);
}

// from_fixed (fixed.rs:81-86) of a stored value v != 0 (0 is the NaN code), in the precision of the typed result: the one
// definition store_typed and value_bounds share
K2R_HD float from_fixed_f32(int64_t v, uint32_t fbits) { return (float)(v - 1) / (float)((int64_t)1 << (fbits + 1)); }
K2R_HD double from_fixed_f64(int64_t v, uint32_t fbits) { return (double)(v - 1) / (double)((int64_t)1 << (fbits + 1)); }

// MMBuffer3::set conversions (mmbuffer.rs:505,525,560,622; fixed.rs:81-86)
K2R_HD void store_typed(void* out, int64_t off, int32_t dtype, int64_t v, uint32_t fbits) {
    switch (dtype) {
        case ENC_I32: ((int32_t*)out)[off] = (int32_t)v; break;
        case ENC_I64: ((int64_t*)out)[off] = v; break;
        case ENC_F32: {
            float f;
            if (v == 0) f = __builtin_nanf("");
            else f = from_fixed_f32(v, fbits);
            ((float*)out)[off] = f;
            break;
        }
        default: {
            double f;
            if (v == 0) f = __builtin_nan("");
            else f = from_fixed_f64(v, fbits);
            ((double*)out)[off] = f;
            break;
        }
    }
}

// ---- value search: real-valued bounds -> the stored integers that match --------------------------------------------------
// A cell matches [lower, upper] iff the value the typed fill_window returns for it, v, satisfies lower <= v <= upper exactly:
// v = from_fixed in the chunk's float type (NaN for stored 0: never a match) or the stored integer itself.  v is monotone
// non-decreasing in the stored n (rounding is monotone), so the matching n form one interval [lo, hi], less n = 0 for floats
// when the interval holds it (`hole`, normalised so that it is only set when lo < 0 < hi).  float32 collapses many n into one
// value once |n - 1| > 2^24, so the ends are found by bisection with the decoder's own expression, not by a closed form.
// 62 fractional bits: from_fixed's divisor (int64_t)1 << 63 is -2^63 (the reference's too, fixed.rs:84), so the decoded
// value is -(n - 1) / 2^63, non-INCREASING in n.  The matching n still form one interval: the bisection runs on -v(n), which
// is non-decreasing, against the mirrored bounds [-upper, -lower].
struct ValueRange {
    int64_t lo, hi;
    bool hole;   // stored 0 lies in [lo, hi] and is not a match
    bool empty;  // nothing matches (lo > hi)
};
// v(n) >= x (ge) or v(n) > x (!ge), exactly: a float32 value converts to double exactly
K2R_HD bool vb_above(int32_t enc, uint32_t fbits, int64_t n, double x, bool ge) {
    double v = enc == ENC_F32 ? (double)from_fixed_f32(n, fbits) : from_fixed_f64(n, fbits);
    if (fbits == 62) v = -v;  // (the wrapped divisor: see above; x is a mirrored bound then)
    return ge ? v >= x : v > x;
}
// the smallest n of [INT64_MIN + 1, INT64_MAX] with vb_above(n) (the predicate is monotone in n); *none when there is none
K2R_HD int64_t vb_first(int32_t enc, uint32_t fbits, double x, bool ge, bool* none) {
    int64_t lo = INT64_MIN + 1, hi = INT64_MAX;  // (INT64_MIN - 1 overflows in from_fixed; to_fixed never stores INT64_MIN)
    *none = !vb_above(enc, fbits, hi, x, ge);
    if (*none) return 0;
    while (lo < hi) {  // at most 64 steps
        const int64_t mid = lo + (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1);
        if (vb_above(enc, fbits, mid, x, ge)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// false: bad argument (a NaN bound, an unknown encoding, float fractional bits beyond what from_fixed defines: > 62, the
// limit Chunk::build enforces).  Reversed bounds are swapped; +-inf is unbounded.
K2R_HD bool value_bounds(int32_t enc, uint32_t fbits, double lower, double upper, ValueRange* r) {
    r->lo = 1;
    r->hi = 0;
    r->hole = false;
    r->empty = true;
    if (lower != lower || upper != upper) return false;
    if (enc != ENC_I32 && enc != ENC_I64 && enc != ENC_F32 && enc != ENC_F64) return false;
    if ((enc == ENC_F32 || enc == ENC_F64) && fbits > 62) return false;
    if (lower > upper) {
        const double x = lower;
        lower = upper;
        upper = x;
    }
    int64_t lo, hi;
    constexpr double two63 = 9223372036854775808.0;
    if (enc == ENC_I32 || enc == ENC_I64) {  // n in [ceil(lower), floor(upper)]; n itself is never rounded to double
        const double cl = __builtin_ceil(lower), fu = __builtin_floor(upper);
        if (cl >= two63 || fu < -two63) return true;
        lo = cl <= -two63 ? INT64_MIN : (int64_t)cl;
        hi = fu >= two63 ? INT64_MAX : (int64_t)fu;
        if (enc == ENC_I32) {
            if (lo < INT32_MIN) lo = INT32_MIN;
            if (hi > INT32_MAX) hi = INT32_MAX;
        }
    } else {
        if (fbits == 62) {  // v(n) = -(n - 1) / 2^63: lower <= v <= upper  <=>  -upper <= -v <= -lower
            const double x = -upper;
            upper = -lower;
            lower = x;
        }
        bool none = false;
        if (lower == -__builtin_inf()) {
            lo = INT64_MIN;
        } else {
            lo = vb_first(enc, fbits, lower, true, &none);  // min{n : v(n) >= lower}
            if (none) return true;
        }
        if (upper == __builtin_inf()) {
            hi = INT64_MAX;
        } else {
            const int64_t above = vb_first(enc, fbits, upper, false, &none);  // max{n : v(n) <= upper} = min{n : v(n) > upper} - 1
            if (none) hi = INT64_MAX;
            else if (above == INT64_MIN + 1) return true;
            else hi = above - 1;
        }
        if (lo <= 0 && 0 <= hi) {  // the NaN code: only a hole strictly inside the interval stays a hole
            if (lo == 0 && hi == 0) return true;
            if (lo == 0) lo = 1;
            else if (hi == 0) hi = -1;
            else r->hole = true;
        }
    }
    if (lo > hi) {
        r->hole = false;
        return true;
    }
    r->lo = lo;
    r->hi = hi;
    r->empty = false;
    return true;
}

}  // namespace k2r
