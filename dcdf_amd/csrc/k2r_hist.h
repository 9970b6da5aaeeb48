// k2r_hist.h -- per-instant value histograms (dcdf_raster_histogram_batch): what the planner (k2r_plan.h), the bulk kernel
// (k2r_bulk.hip) and the fold kernel share.  Everything above the plan compiles for the host alone as well (g++), so the
// translation of bin edges into stored integers can be run and sanitised on a CPU.
//
// The contract (include/dcdf_k2r.h): per instant, over the selected cells of a cube, x = reduce_widen of
// the stored integer; a non-NaN x is counted in bin b when edges[b] <= x < edges[b + 1], the last bin taking x == edges[n_bins]
// as well (numpy.histogram's rule for explicit edges).  Counts are integers: any cut and any order of the work give one result.
//
// Why integer compares do it: x is a monotone function of the stored integer n within one leaf (rounding is monotone), so the
// n of one bin form one interval, and an edge becomes "the first n whose x reaches it".  No closed form gives that n where the
// decoder rounds -- (double)n beyond 2^53, (float)(n - 1) beyond 2^24 -- so it is found by bisection with the decoder's own
// expression, vb_first's method (k2r_decode.h).  With 62 fractional bits from_fixed's divisor is -2^63 and x is non-INCREASING in
// n: the bisection runs on -x, the edges are mirrored, which swaps the strictness of every comparison and reverses the bins.
#pragma once
#include "k2r_decode.h"

namespace k2r {

constexpr uint32_t HIST_MAX_BINS = 256;  // DCDF_HIST_MAX_BINS

K2R_HD bool hist_float(int32_t enc) { return enc == ENC_F32 || enc == ENC_F64; }
K2R_HD bool hist_reversed(int32_t enc, uint32_t fbits) { return hist_float(enc) && fbits == 62u; }
// the stored integers a leaf can hold (INT64_MIN - 1 overflows in from_fixed; to_fixed never stores INT64_MIN)
K2R_HD int64_t hist_dom_lo(int32_t enc) { return enc == ENC_I32 ? (int64_t)INT32_MIN : enc == ENC_I64 ? INT64_MIN : INT64_MIN + 1; }
K2R_HD int64_t hist_dom_hi(int32_t enc) { return enc == ENC_I32 ? (int64_t)INT32_MAX : INT64_MAX; }
// reduce_widen (k2r_reduce.h) of n -- for a float leaf of n != 0; n = 0 is the NaN code and is left out by the callers -- negated
// where it decreases in n, so that the key is non-decreasing over the leaf's stored integers
K2R_HD double hist_key(int32_t enc, uint32_t fbits, int64_t n) {
    switch (enc) {
        case ENC_I32: return (double)(int32_t)n;
        case ENC_I64: return (double)n;
        case ENC_F32: {
            const double v = (double)from_fixed_f32(n, fbits);
            return fbits == 62u ? -v : v;
        }
        default: {
            const double v = from_fixed_f64(n, fbits);
            return fbits == 62u ? -v : v;
        }
    }
}
// the smallest stored integer with key >= x (ge) or key > x (!ge); *none when there is none
K2R_HD int64_t hist_first(int32_t enc, uint32_t fbits, double x, bool ge, bool* none) {
    int64_t lo = hist_dom_lo(enc), hi = hist_dom_hi(enc);
    const double top = hist_key(enc, fbits, hi);
    *none = !(ge ? top >= x : top > x);
    if (*none) return 0;
    while (lo < hi) {  // at most 64 steps
        const int64_t mid = lo + (int64_t)(((uint64_t)hi - (uint64_t)lo) >> 1);
        const double v = hist_key(enc, fbits, mid);
        if (ge ? v >= x : v > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// Edge j of n_bins + 1 as a threshold on stored integers: x >= edges[j] (the last edge: x > edges[n_bins]) exactly for the n
// from the threshold on.  Reversed leaves: x <= edges[j] (the last edge: x < edges[n_bins]) from the threshold on.
K2R_HD int64_t hist_threshold(int32_t enc, uint32_t fbits, const double* edges, uint32_t n_bins, uint32_t j, bool* none) {
    if (hist_reversed(enc, fbits)) return hist_first(enc, fbits, -edges[j], j == n_bins, none);
    return hist_first(enc, fbits, edges[j], j != n_bins, none);
}
// n_bins in range, no NaN, strictly increasing
K2R_HD bool hist_edges_ok(const double* edges, uint32_t n_bins) {
    if (!edges || n_bins == 0 || n_bins > HIST_MAX_BINS) return false;
    for (uint32_t j = 0; j <= n_bins; j++) {
        if (edges[j] != edges[j]) return false;
        if (j && !(edges[j - 1] < edges[j])) return false;
    }
    return true;
}
K2R_HD bool hist_leaf_ok(int32_t enc, uint32_t fbits) {
    if (enc != ENC_I32 && enc != ENC_I64 && enc != ENC_F32 && enc != ENC_F64) return false;
    return !(hist_float(enc) && fbits > 62u);
}
// [lo[b], hi[b]]: the stored integers of bin b, lo[b] > hi[b] (1, 0) when there is none.  The NaN code 0 of a float leaf is
// never an end of an interval; strictly inside one it is simply never counted.
K2R_HD void hist_intervals(int32_t enc, uint32_t fbits, const double* edges, uint32_t n_bins, int64_t* lo, int64_t* hi) {
    const bool rev = hist_reversed(enc, fbits);
    for (uint32_t b = 0; b < n_bins; b++) {
        bool none_a = false, none_b = false;
        const int64_t a = hist_threshold(enc, fbits, edges, n_bins, rev ? b + 1u : b, &none_a);      // the bin's first integer
        const int64_t e = hist_threshold(enc, fbits, edges, n_bins, rev ? b : b + 1u, &none_b);      // the first one beyond it
        lo[b] = 1;
        hi[b] = 0;
        if (none_a || (!none_b && e == hist_dom_lo(enc))) continue;
        int64_t l = a, h = none_b ? hist_dom_hi(enc) : e - 1;
        if (hist_float(enc)) {
            if (l == 0) l = 1;
            if (h == 0) h = -1;
        }
        if (l > h) continue;
        lo[b] = l;
        hi[b] = h;
    }
}
// The thresholds of a leaf for the bulk kernel, whose stored integers are int32 (narrow32 chunks): ascending, clamped, "none" =
// INT32_MAX (beyond every value of such a chunk), padded with INT32_MAX to `size` entries.  With p = (the number of entries
// <= n) - 1, n falls in bin p -- reversed leaves: n_bins - 1 - p -- when 0 <= p < n_bins, and in none otherwise.
K2R_HD void hist_thresholds32(int32_t enc, uint32_t fbits, const double* edges, uint32_t n_bins, int32_t* thr, uint32_t size) {
    const bool rev = hist_reversed(enc, fbits);
    for (uint32_t i = 0; i < size; i++) {
        int32_t v = INT32_MAX;
        if (i <= n_bins) {
            bool none = false;
            const int64_t t = hist_threshold(enc, fbits, edges, n_bins, rev ? n_bins - i : i, &none);
            if (!none) v = t < (int64_t)INT32_MIN ? INT32_MIN : t > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)t;
        }
        thr[i] = v;
    }
}
// steps of the branch-free search over the thresholds: the table holds 2^steps entries, more than n_bins + 1
K2R_HD uint32_t hist_steps(uint32_t n_bins) {
    uint32_t k = 1;
    while (((uint32_t)1 << k) < n_bins + 2u) k++;
    return k;
}
// p of hist_thresholds32: entries <= n, less one (the table's last entry is padding, never counted)
K2R_HD int32_t hist_search32(const int32_t* thr, uint32_t steps, int32_t n) {
    uint32_t pos = 0;
    for (uint32_t s = (uint32_t)1 << (steps - 1u); s; s >>= 1) pos += thr[pos + s - 1u] <= n ? s : 0u;
    return (int32_t)pos - 1;
}
// the bin of a value, by the definition itself (the fold kernel, the elided pieces): -1 for NaN and for a value outside the edges
K2R_HD int32_t hist_bin(const double* edges, uint32_t n_bins, double x) {
    if (!(x >= edges[0] && x <= edges[n_bins])) return -1;
    uint32_t lo = 0, hi = n_bins;  // edges[lo] <= x, and x < edges[hi] or hi = n_bins
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (edges[mid] <= x) lo = mid;
        else hi = mid;
    }
    return (int32_t)lo;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// One workgroup's work in k_bulk_hist: BulkUnit (k2r_bulk.h) with the place of its instants' rows in the output, of its cells'
// mask bytes and of its leaf's thresholds instead of the output strides.  The counts of instant t go to out[o_off + (t - t0) *
// n_bins + bin].
struct HistUnit {
    uint32_t chunk;  // index into the ChunkRef table
    uint32_t t0, t1;
    uint16_t rr, rc;
    uint16_t top, bottom, left, right;
    uint32_t m_sr;   // row stride of the mask in bytes (the cube's columns)
    uint32_t thr;    // first entry of the leaf's thresholds in the table (hist_thresholds32)
    uint32_t rev;    // the leaf's bins run against its stored integers (hist_reversed)
    uint32_t _pad;
    uint64_t o_off;
    uint64_t m_off;  // mask byte of cell (top, left)
};
// A fallback or elided piece folded by k_hist_fold.  src: element of (first instant, first row, first column) in the slab of
// stored integers, dense [nt][rows][cols]; for an elided piece the index of its first instant in dcdf_raster::d_vals.  The
// counts of the piece's instant i go to out[o_off + i * n_bins + bin].
struct HistFold {
    uint32_t nt, rows, cols, m_sr;
    int32_t enc;
    uint32_t fbits, elided, _pad;
    uint64_t src, o_off, m_off;
};

#if defined(__HIPCC__)
struct ChunkRef;
// k_bulk_hist over n units on the null stream (asynchronous).  d_enc: the chunks' encodings; d_mask: the masks' bytes or null;
// d_thr: the leaves' threshold tables, 2^hist_steps(n_bins) entries each; d_out: the zeroed accumulator.  Returns a DCDF code.
int launch_bulk_hist(const ChunkRef* d_refs, const uint8_t* d_enc, const HistUnit* d_units, uint32_t n, const uint8_t* d_mask,
                     const int32_t* d_thr, uint32_t n_bins, uint64_t* d_out);
#endif

}  // namespace k2r
