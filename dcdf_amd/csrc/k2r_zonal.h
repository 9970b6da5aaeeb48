// k2r_zonal.h -- zonal statistics (dcdf_raster_zonal_batch): what the planner (k2r_plan.h), the bulk kernel (k2r_bulk.hip) and
// the fold / finish kernels share.  The arithmetic compiles for the host alone as well (g++), as k2r_space.h's does: the tests run
// and sanitise it on a CPU (tests/sim/zonal_check.cpp).
//
// The contract (include/dcdf_k2r.h): one uint16 label per cell of a cube; per (zone, instant) the
// statistics of dcdf_raster_reduce_space_batch over the cells that carry the zone's label.  One walk of the encoded bytes serves
// every zone: a batch keeps one accumulator entry per (cube, zone, instant) in device scratch, every piece of the work adds to it
// with integer atomics alone -- commutative and associative, so the result depends on no order and on no cut of the work -- and
// k_zonal_finish turns the entries into the cubes' matrices.
#pragma once
#include "k2r_space.h"

namespace k2r {

constexpr uint32_t ZONAL_NONE = 0xffffu;  // DCDF_ZONE_NONE: the label of no zone (as is every label >= n_zones)
constexpr uint32_t ZONAL_ZL = 16;         // zone slots of k_bulk_zonal's LDS accumulators: distinct labels of a unit per round
constexpr uint32_t ZONAL_B = 16;          // instants whose LDS accumulators wait for one flush
constexpr uint32_t ZONAL_MAX_LABELS = 65536;
constexpr uint32_t ZONAL_BM_WORDS = ZONAL_MAX_LABELS / 32;  // the label bitmap of a unit: 8 KB

// ---- one accumulator entry: 9 words of 64 bits, all zero = "nothing yet" -----------------------------------------------------
//   [0]      the count of non-NaN values                                                      (atomic add)
//   [1]      ~key of the minimum, [2] key of the maximum: zonal_key below, 0 = none           (atomic unsigned max)
//   [3 + i]  limb i of the sum at the 2^-63 scale, i < 6: an int64 counter                    (atomic add)
constexpr uint32_t ZA_CNT = 0, ZA_MIN = 1, ZA_MAX = 2, ZA_LIMB = 3, ZONAL_WORDS = 9;
constexpr uint64_t ZONAL_BYTES = 8u * ZONAL_WORDS;  // 72: the planner sizes the scratch by it

// The order-preserving key of a double: unsigned compare of keys = numeric compare of the doubles, with -0.0 below +0.0 (the
// contract's rule for a zone that holds both).  No value has the key 0 or ~0 (they are NaNs with a full payload), so 0 can say
// "none" for the maximum and, inverted, for the minimum.
K2R_HD uint64_t zonal_key(double d) {
    uint64_t b;
    __builtin_memcpy(&b, &d, sizeof b);
    return (b >> 63) ? ~b : b | ((uint64_t)1 << 63);
}
K2R_HD double zonal_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? k & ~((uint64_t)1 << 63) : ~k;
    double d;
    __builtin_memcpy(&d, &b, sizeof d);
    return d;
}

// ---- the sum in limbs --------------------------------------------------------------------------------------------------------
// v (two's complement, 192 bits) = sum of limb[i] * 2^(32 i): the low five limbs unsigned 32-bit values, the top one signed.
// Each is added to its own int64 counter, which absorbs 2^31 such additions; a zone-instant receives at most one per piece.
K2R_HD int64_t zonal_limb(const U192& v, uint32_t i) {
    const uint64_t w = i < 2u ? v.w0 : i < 4u ? v.w1 : v.w2;
    const uint32_t h = (uint32_t)((i & 1u) ? w >> 32 : w);
    return i == 5u ? (int64_t)(int32_t)h : (int64_t)h;
}
// The counters back into one integer: sum of limbs[i] * 2^(32 i), any int64 counters, formed in 256 bits.  False when the value
// is not a 192-bit two's complement integer (space_round's domain, |v| < 2^191: far beyond what 2^32 cells of |x| <= 1 reach).
K2R_HD bool zonal_fold(const int64_t (&limbs)[6], U192& out) {
    uint64_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 6u; i++) {
        const uint64_t lo = (uint64_t)limbs[i], ext = limbs[i] < 0 ? ~(uint64_t)0 : (uint64_t)0;
        const uint32_t wi = i >> 1;
        uint64_t a[4];  // limbs[i] sign-extended to 256 bits and shifted left by 32 i
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint64_t cur = k < wi ? 0u : k == wi ? lo : ext;           // word k - wi of the extended value
            const uint64_t below = k < wi + 1u ? 0u : k == wi + 1u ? lo : ext;  // word k - wi - 1
            a[k] = (i & 1u) ? (cur << 32) | (below >> 32) : cur;
        }
        uint64_t carry = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint64_t s = w[k] + a[k], c1 = s < w[k] ? 1u : 0u;
            const uint64_t t = s + carry, c2 = t < s ? 1u : 0u;
            w[k] = t;
            carry = c1 + c2;
        }
    }
    out = U192{w[0], w[1], w[2]};
    return w[3] == ((w[2] >> 63) ? ~(uint64_t)0 : (uint64_t)0);
}

// ---- the distinct labels of a unit, ranked ------------------------------------------------------------------------------------
// bm: a bitmap of ZONAL_BM_WORDS words with the bit of every label the unit's selected cells carry; pre[w] = the number of set bits
// in the words before w.  The rank of a label among the distinct ones, ascending (np.unique's place), is then one lookup.  A
// workgroup of 256 threads builds pre in three steps: thread t counts its 8 words (zonal_count8), the counts are scanned
// (exclusively) over the threads, thread t writes its words' entries from its own start (zonal_prefix8).
K2R_HD uint32_t zonal_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
K2R_HD uint32_t zonal_count8(const uint32_t* bm, uint32_t t) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) n += zonal_popc(bm[8u * t + j]);
    return n;
}
K2R_HD void zonal_prefix8(const uint32_t* bm, uint32_t* pre, uint32_t t, uint32_t start) {
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        pre[8u * t + j] = start;
        start += zonal_popc(bm[8u * t + j]);
    }
}
K2R_HD uint32_t zonal_rank(const uint32_t* bm, const uint32_t* pre, uint32_t label) {
    return pre[label >> 5] + zonal_popc(bm[label >> 5] & (((uint32_t)1 << (label & 31u)) - 1u));
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// One workgroup's work in k_bulk_zonal: BulkUnit's first 24 bytes (k2r_bulk.h), the place of its cells' labels, and its
// accumulators: entry (zone z, instant t) is acc + z * a_st + (t - t0).
struct ZonalUnit {
    uint32_t chunk;  // index into the ChunkRef table
    uint32_t t0, t1;
    uint16_t rr, rc;
    uint16_t top, bottom, left, right;
    uint32_t m_sr;   // row stride of the labels in elements (the cube's columns)
    uint32_t a_st;   // zone stride of the accumulators in entries (the instants of the unit's span)
    uint64_t acc;
    uint64_t m_off;  // label element of cell (top, left)
};
// A fallback or elided piece folded by k_zonal_fold: SpaceFold's fields, with the accumulators instead of the records.
struct ZonalFold {
    uint32_t nt, rows, cols, m_sr;
    int32_t enc;
    uint32_t fbits, elided, a_st;
    uint64_t src, acc, m_off;
};
// The instants [a, a + nt) of one cube, whose accumulators are the entries acc + z * nt + i of the batch's scratch; statistic k of
// (zone z, instant i) goes to dst[o_off + k * o_stat + z * o_zone + i].
struct ZonalSpan {
    uint64_t acc;
    uint32_t nt, _pad;
    uint64_t o_off, o_zone, o_stat;
};

#if defined(__HIPCC__)
struct ChunkRef;
// One piece's statistics of one (zone, instant) into its entry e: the sum (hi, lo) at the leaf's scale, cnt non-NaN values, their
// extremes already widened.  Device-scope atomics on 64-bit words; only what `live` (RA_*, k2r_reduce.h) carries.
__device__ __forceinline__ void zonal_add(uint64_t* acc, uint64_t e, uint64_t hi, uint64_t lo, uint32_t scale, uint64_t cnt, double mn, double mx,
                                          bool ext, bool add) {
    __attribute__((address_space(1))) unsigned long long* const A = (__attribute__((address_space(1))) unsigned long long*)acc + e * ZONAL_WORDS;
    __hip_atomic_fetch_add(A + ZA_CNT, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ext) {
        __hip_atomic_fetch_max(A + ZA_MIN, (unsigned long long)~zonal_key(mn), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(A + ZA_MAX, (unsigned long long)zonal_key(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (add) {
        const U192 v = space_scaled(hi, lo, scale);
#pragma unroll
        for (uint32_t i = 0; i < 6u; i++) {
            const int64_t l = zonal_limb(v, i);
            if (l != 0) __hip_atomic_fetch_add(A + ZA_LIMB + i, (unsigned long long)l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// k_bulk_zonal over n units on the null stream (asynchronous).  d_enc: the chunks' encodings; d_labels: the cubes' labels;
// live: the accumulators the statistics need (reduce_live, k2r_reduce.h).  Returns a DCDF code.
int launch_bulk_zonal(const ChunkRef* d_refs, const uint8_t* d_enc, const ZonalUnit* d_units, uint32_t n, const uint16_t* d_labels,
                      uint32_t n_zones, uint64_t* d_acc, uint32_t live);
#endif

}  // namespace k2r
