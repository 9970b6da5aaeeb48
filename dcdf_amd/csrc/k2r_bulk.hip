// k2r_bulk.hip -- the eight bulk kernels over whole regions of a stored raster: decode (k2r_bulk.h), reduction over time
// (k2r_reduce.h), grouped reduction over time (k2r_group.h), moments over time (k2r_moment.h), reduction over space (k2r_space.h),
// value histograms (k2r_hist.h), spell statistics (k2r_spell.h), zonal statistics (k2r_zonal.h).  All eight
// walk a unit the same way; that walk, and why it yields fill_window's values, is in k2r_bulk_walk.h (bulk_instant, bulk_cells8,
// bulk_select16).  A thread gets the same 16 cells of the region at every instant; what is here is what each kernel does with them.
#include <hip/hip_runtime.h>

#include "k2r_bulk_walk.h"
#include "k2r_group.h"
#include "k2r_hist.h"
#include "k2r_moment.h"
#include "k2r_reduce.h"
#include "k2r_runtime.h"
#include "k2r_space.h"
#include "k2r_spell.h"
#include "k2r_zonal.h"

namespace k2r {

// MMBuffer3::set's conversions (store_typed, k2r_decode.h) for four cells of one row: chunk row r, columns c0 .. c0 + 3 (c0 a
// multiple of 4), clipped to [left, right); `off` = element of (r, c0) in out.  One 16-byte store (two for 8-byte elements) when the
// four cells are inside and the destination is aligned, single elements otherwise.
template <int DT>
__device__ __forceinline__ void bulk_store4(void* out, int64_t off, const int32_t (&v)[4], uint32_t c0, uint32_t left, uint32_t right, uint32_t fbits) {
    const bool full = c0 >= left && c0 + 4u <= right;
    if constexpr (DT == ENC_I32 || DT == ENC_F32) {
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if constexpr (DT == ENC_I32) {
                w[e] = (uint32_t)v[e];
            } else {
                const float f = v[e] == 0 ? __builtin_nanf("") : from_fixed_f32((int64_t)v[e], fbits);
                w[e] = __builtin_bit_cast(uint32_t, f);
            }
        }
        uint32_t* const p = (uint32_t*)out + off;
        if (full && ((uintptr_t)p & 15u) == 0) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            *(__attribute__((address_space(1))) u32x4*)p = u32x4{w[0], w[1], w[2], w[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (c0 + (uint32_t)e >= left && c0 + (uint32_t)e < right) ((__attribute__((address_space(1))) uint32_t*)p)[e] = w[e];
        }
    } else {
        uint64_t w[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if constexpr (DT == ENC_I64) {
                w[e] = (uint64_t)(int64_t)v[e];
            } else {
                const double f = v[e] == 0 ? __builtin_nan("") : from_fixed_f64((int64_t)v[e], fbits);
                w[e] = __builtin_bit_cast(uint64_t, f);
            }
        }
        uint64_t* const p = (uint64_t*)out + off;
        if (full && ((uintptr_t)p & 15u) == 0) {
            typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
            *(__attribute__((address_space(1))) u64x2*)p = u64x2{w[0], w[1]};
            *(__attribute__((address_space(1))) u64x2*)(p + 2) = u64x2{w[2], w[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (c0 + (uint32_t)e >= left && c0 + (uint32_t)e < right) ((__attribute__((address_space(1))) uint64_t*)p)[e] = w[e];
        }
    }
}

// V: the walk's value type.  A chunk with a side-16 table whose values lie in [-2^30, 2^30) has every node extreme and every Log
// difference in int32 (dcdf_chunk::narrow32); only such chunks come here.  DT: the output's dtype.
template <class V, int DT>
__global__ void __launch_bounds__(256)
k_bulk_decode(const ChunkRef* __restrict__ chunks, const BulkUnit* __restrict__ units, uint32_t n_units, void* out) {
    static_assert(sizeof(V) == 4, "the pyramid holds 32-bit values");
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];  // the Snapshot's first-child indices while the pyramid is built, then the Log walk's state
    __shared__ V nd[BN_SIZE];
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const BulkUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const gbytes gb = (gbytes)C.bytes;
        const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
        uint32_t cur_snap = 0xffffffffu;
        for (uint32_t t = U.t0; t < U.t1; t++) {
            const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
            // ---- nodes of side 2, two per task: their 2 x 4 cells, stored as two row segments ----
            const int64_t obase = (int64_t)U.out_off + (int64_t)(t - U.t0) * (int64_t)U.out_st - (int64_t)top * U.out_sr - (int64_t)left;
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                const uint32_t r0 = (uint32_t)U.rr + 2u * rp, c0 = (uint32_t)U.rc + 4u * cg;  // chunk coordinates
                if (r0 + 2u <= top || r0 >= bottom || c0 + 4u <= left || c0 >= right) continue;
                V v[2][4];
                bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                for (uint32_t i = 0; i < 2u; i++) {
                    const uint32_t r = r0 + i;
                    if (r < top || r >= bottom) continue;
                    bulk_store4<DT>(out, obase + (int64_t)r * U.out_sr + (int64_t)c0, v[i], c0, left, right, C.fbits);
                }
            }
        }
        __syncthreads();
    }
}

uint32_t bulk_wanted_units() {
    const int cus = Runtime::get().cus;
    return 4u * (uint32_t)(cus > 0 ? cus : 256);
}

int launch_bulk_decode(const ChunkRef* d_refs, const BulkUnit* d_units, uint32_t n, void* d_out, int32_t out_dtype) {
    if (n == 0) return DCDF_OK;
    const dim3 grid = bulk_grid(n), block(256);
    switch (out_dtype) {
        case DCDF_I32: hipLaunchKernelGGL((k_bulk_decode<int32_t, ENC_I32>), grid, block, 0, 0, d_refs, d_units, n, d_out); break;
        case DCDF_I64: hipLaunchKernelGGL((k_bulk_decode<int32_t, ENC_I64>), grid, block, 0, 0, d_refs, d_units, n, d_out); break;
        case DCDF_F32: hipLaunchKernelGGL((k_bulk_decode<int32_t, ENC_F32>), grid, block, 0, 0, d_refs, d_units, n, d_out); break;
        case DCDF_F64: hipLaunchKernelGGL((k_bulk_decode<int32_t, ENC_F64>), grid, block, 0, 0, d_refs, d_units, n, d_out); break;
        default: return DCDF_ERR_BAD_ARG;
    }
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- what the folding kernels know of a leaf's encoding --------------------------------------------------------------------
// 0: an integer leaf, x = (double)n.  1 / 2: a float32 / float64 leaf, stored 0 is NaN and x = from_fixed(n) (k2r_decode.h).
__device__ __forceinline__ int leaf_kind(int32_t enc) { return enc == ENC_F32 ? 1 : enc == ENC_F64 ? 2 : 0; }
// The sign mirror of a leaf's stored integers: key = (n ^ sg) - sg is n for sg = 0, -n for sg = -1, and its own inverse.
// from_fixed is monotone in n, so a unit keeps its extremes as keys and widens them once.  x DEcreases in n exactly when
// from_fixed's divisor (int64_t)1 << (fbits + 1) is negative: the shift into the sign bit, fbits == 62 (no leaf has more).
__device__ __forceinline__ int32_t leaf_mirror(int kind, uint32_t fbits) { return kind != 0 && fbits == 62u ? -1 : 0; }
// a unit's extreme from its key: NaN while the key is still at its sentinel `none` ("no value yet"), else the contract's x
__device__ __forceinline__ double leaf_extreme(int32_t key, int32_t none, int32_t enc, uint32_t fbits, int32_t sg) {
    return key == none ? __builtin_nan("") : reduce_widen(enc, fbits, (int64_t)((key ^ sg) - sg));
}

// ---- reduction over time (k2r_reduce.h): the walk's cells into per-cell accumulators ----------------------------------------
// Four cells of one row of a state plane: p = element of chunk column c0 (a multiple of 4), clipped to [left, right).  Two
// 16-byte accesses when the four cells are inside and p is aligned, single elements otherwise (bulk_store4's rule).
typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void plane_load4(const double* p, double (&v)[4], uint32_t c0, uint32_t left, uint32_t right) {
    if (c0 >= left && c0 + 4u <= right && ((uintptr_t)p & 15u) == 0) {
        const f64x2 a = *(const __attribute__((address_space(1))) f64x2*)p, b = *(const __attribute__((address_space(1))) f64x2*)(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c0 + (uint32_t)e >= left && c0 + (uint32_t)e < right) v[e] = ((const __attribute__((address_space(1))) double*)p)[e];
    }
}
__device__ __forceinline__ void plane_store4(double* p, const double (&v)[4], uint32_t c0, uint32_t left, uint32_t right) {
    if (c0 >= left && c0 + 4u <= right && ((uintptr_t)p & 15u) == 0) {
        *(__attribute__((address_space(1))) f64x2*)p = f64x2{v[0], v[1]};
        *(__attribute__((address_space(1))) f64x2*)(p + 2) = f64x2{v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c0 + (uint32_t)e >= left && c0 + (uint32_t)e < right) ((__attribute__((address_space(1))) double*)p)[e] = v[e];
    }
}
// One instant of four cells into their accumulators.  KIND 0: an integer chunk, x = (double)n.  KIND 1 / 2: a float32 / float64
// chunk, stored 0 is NaN and skipped, x = from_fixed (k2r_decode.h) with the division by +-2^(fbits + 1) written as the product
// with its reciprocal (inv / invf): both are exact, so the bits are from_fixed's.  lo / hi hold the extremes as stored integers
// (keys mirrored by sg, leaf_mirror) and are converted once per unit.
template <uint32_t LIVE, int KIND>
__device__ __forceinline__ void reduce_fold4(const int32_t (&v)[4], double (&s)[4], uint32_t (&cnt)[4], int32_t (&lo)[4], int32_t (&hi)[4],
                                             double inv, float invf, int32_t sg) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int32_t n = v[e];
        if constexpr (KIND == 0) {
            if constexpr ((LIVE & RA_SUM) != 0) s[e] = s[e] + (double)n;
            if constexpr ((LIVE & RA_MIN) != 0) lo[e] = n < lo[e] ? n : lo[e];
            if constexpr ((LIVE & RA_MAX) != 0) hi[e] = n > hi[e] ? n : hi[e];
        } else {
            const bool ok = n != 0;
            if constexpr ((LIVE & RA_SUM) != 0) {
                const double x = KIND == 1 ? (double)((float)(n - 1) * invf) : (double)(n - 1) * inv;
                const double a = s[e] + x;
                s[e] = ok ? a : s[e];
            }
            if constexpr ((LIVE & RA_COUNT) != 0) cnt[e] += ok ? 1u : 0u;
            const int32_t key = (n ^ sg) - sg;
            if constexpr ((LIVE & RA_MIN) != 0) lo[e] = ok && key < lo[e] ? key : lo[e];
            if constexpr ((LIVE & RA_MAX) != 0) hi[e] = ok && key > hi[e] ? key : hi[e];
        }
    }
}

// LIVE: the accumulators this instantiation carries (RA_*).  A thread owns the same 16 cells at every instant (its two tasks
// of 2 rows x 4 columns, bulk_cells8); their accumulators stay in registers over the unit's instants.  SUM continues the chain
// of the state plane: it is loaded before the first instant (0.0 when the unit starts its cube) and stored after the last.
// COUNT, MIN and MAX are merged into their planes at the end (identity NaN).  Cells outside the unit's rectangle are decoded as
// in k_bulk_decode; their rows are not accumulated and nothing of them is written.
template <uint32_t LIVE>
__global__ void __launch_bounds__(256)
k_bulk_reduce(const ChunkRef* __restrict__ chunks, const uint8_t* __restrict__ encs, const ReduceUnit* __restrict__ units, uint32_t n_units,
              double* dst, double* scr, uint32_t ops) {
    typedef int32_t V;
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const ReduceUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const int32_t enc = (int32_t)encs[U.chunk];
        const int kind = leaf_kind(enc);
        const int64_t div = (int64_t)1 << (C.fbits + 1u);  // from_fixed's divisor
        const double inv = 1.0 / (double)div;
        const float invf = 1.0f / (float)div;
        const int32_t sg = leaf_mirror(kind, C.fbits);
        const gbytes gb = (gbytes)C.bytes;
        const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
        double* const p_min = reduce_plane(RA_MIN, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_max = reduce_plane(RA_MAX, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_sum = reduce_plane(RA_SUM, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_cnt = reduce_plane(RA_COUNT, dst, scr, ops, U.o_off, U.s_off, U.psz);
        // accumulators of row 2 k + i of the thread's cells
        double sum[4][4];
        uint32_t cnt[4][4];
        int32_t lo[4][4], hi[4][4];
#pragma unroll
        for (uint32_t a = 0; a < 4u; a++) {
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                sum[a][e] = 0.0;
                cnt[a][e] = 0u;
                lo[a][e] = INT32_MAX;  // (beyond every stored value of a narrow32 chunk: "no value yet")
                hi[a][e] = INT32_MIN;
            }
            if constexpr ((LIVE & RA_SUM) != 0) {
                const uint32_t g = tid + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
                if (!U.init && r >= top && r < bottom && c0 + 4u > left && c0 < right)
                    plane_load4(p_sum + (int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left), sum[a], c0, left, right);
            }
        }
        uint32_t cur_snap = 0xffffffffu;
        for (uint32_t t = U.t0; t < U.t1; t++) {
            const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
            // ---- nodes of side 2, two per task: their 2 x 4 cells, folded ----
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                const uint32_t r0 = (uint32_t)U.rr + 2u * rp, c0 = (uint32_t)U.rc + 4u * cg;  // chunk coordinates
                if (r0 + 2u <= top || r0 >= bottom || c0 + 4u <= left || c0 >= right) continue;
                V v[2][4];
                bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                for (uint32_t i = 0; i < 2u; i++) {
                    const uint32_t r = r0 + i, a = 2u * k + i;
                    if (r < top || r >= bottom) continue;
                    if (kind == 0) reduce_fold4<LIVE, 0>(v[i], sum[a], cnt[a], lo[a], hi[a], inv, invf, sg);
                    else if (kind == 1) reduce_fold4<LIVE, 1>(v[i], sum[a], cnt[a], lo[a], hi[a], inv, invf, sg);
                    else reduce_fold4<LIVE, 2>(v[i], sum[a], cnt[a], lo[a], hi[a], inv, invf, sg);
                }
            }
        }
        // ---- the unit's accumulators into the state planes ----
#pragma unroll
        for (uint32_t a = 0; a < 4u; a++) {
            const uint32_t g = tid + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
            if (r < top || r >= bottom || c0 + 4u <= left || c0 >= right) continue;
            const int64_t at = (int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left);
            if constexpr ((LIVE & RA_SUM) != 0) plane_store4(p_sum + at, sum[a], c0, left, right);
            if constexpr ((LIVE & RA_COUNT) != 0) {
                double x[4], old[4] = {0.0, 0.0, 0.0, 0.0};
                if (!U.init) plane_load4(p_cnt + at, old, c0, left, right);
#pragma unroll
                for (uint32_t e = 0; e < 4u; e++) x[e] = old[e] + (double)(kind != 0 ? cnt[a][e] : U.t1 - U.t0);
                plane_store4(p_cnt + at, x, c0, left, right);
            }
            if constexpr ((LIVE & RA_MIN) != 0) {
                double x[4], old[4];
#pragma unroll
                for (uint32_t e = 0; e < 4u; e++) {
                    x[e] = leaf_extreme(lo[a][e], INT32_MAX, enc, C.fbits, sg);
                    old[e] = __builtin_nan("");
                }
                if (!U.init) plane_load4(p_min + at, old, c0, left, right);
#pragma unroll
                for (uint32_t e = 0; e < 4u; e++) x[e] = fmin(old[e], x[e]);
                plane_store4(p_min + at, x, c0, left, right);
            }
            if constexpr ((LIVE & RA_MAX) != 0) {
                double x[4], old[4];
#pragma unroll
                for (uint32_t e = 0; e < 4u; e++) {
                    x[e] = leaf_extreme(hi[a][e], INT32_MIN, enc, C.fbits, sg);
                    old[e] = __builtin_nan("");
                }
                if (!U.init) plane_load4(p_max + at, old, c0, left, right);
#pragma unroll
                for (uint32_t e = 0; e < 4u; e++) x[e] = fmax(old[e], x[e]);
                plane_store4(p_max + at, x, c0, left, right);
            }
        }
        __syncthreads();
    }
}

int launch_bulk_reduce(const ChunkRef* d_refs, const uint8_t* d_enc, const ReduceUnit* d_units, uint32_t n, double* d_dst, double* d_scr,
                       uint32_t ops) {
    if (n == 0) return DCDF_OK;
    const dim3 grid = bulk_grid(n), block(256);
#define K2R_REDUCE_CASE(L) \
    case L: hipLaunchKernelGGL((k_bulk_reduce<L>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_dst, d_scr, ops); break;
    switch (reduce_live(ops)) {
        K2R_REDUCE_CASE(1) K2R_REDUCE_CASE(2) K2R_REDUCE_CASE(3) K2R_REDUCE_CASE(4) K2R_REDUCE_CASE(5)
        K2R_REDUCE_CASE(6) K2R_REDUCE_CASE(7) K2R_REDUCE_CASE(8) K2R_REDUCE_CASE(9) K2R_REDUCE_CASE(10)
        K2R_REDUCE_CASE(11) K2R_REDUCE_CASE(12) K2R_REDUCE_CASE(13) K2R_REDUCE_CASE(14) K2R_REDUCE_CASE(15)
        default: return DCDF_ERR_BAD_ARG;
    }
#undef K2R_REDUCE_CASE
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- grouped reduction over time (k2r_group.h): k_bulk_reduce's accumulators, one run of equal labels at a time ---------------
// The thread's accumulators of one run into the planes of the run's group (p_*: already moved to that group): k_bulk_reduce's
// end-of-unit code with the planes always loaded -- they were filled with the identities before the first segment.  SUM is
// stored (the run began with the plane's value), COUNT added -- for an integer leaf the run's length --, MIN / MAX by fmin / fmax.
template <uint32_t LIVE>
__device__ __forceinline__ void group_merge16(const GroupUnit& U, uint32_t tid, int kind, int32_t enc, uint32_t fbits, int32_t sg, uint32_t run,
                                              double* p_min, double* p_max, double* p_sum, double* p_cnt, const double (&sum)[4][4],
                                              const uint32_t (&cnt)[4][4], const int32_t (&lo)[4][4], const int32_t (&hi)[4][4]) {
    const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
    // The cells' places are worked out again at every merge: hoisted out of the instants' loop they would stay in registers over
    // the walk, which costs a wave per SIMD.
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (uint32_t a = 0; a < 4u; a++) {
        const uint32_t g = tid + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
        if (r < top || r >= bottom || c0 + 4u <= left || c0 >= right) continue;
        const int64_t at = (int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left);
        if constexpr ((LIVE & RA_SUM) != 0) plane_store4(p_sum + at, sum[a], c0, left, right);
        if constexpr ((LIVE & RA_COUNT) != 0) {
            double x[4], old[4] = {0.0, 0.0, 0.0, 0.0};
            plane_load4(p_cnt + at, old, c0, left, right);
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) x[e] = old[e] + (double)(kind != 0 ? cnt[a][e] : run);
            plane_store4(p_cnt + at, x, c0, left, right);
        }
        if constexpr ((LIVE & RA_MIN) != 0) {
            double x[4], old[4];
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                x[e] = leaf_extreme(lo[a][e], INT32_MAX, enc, fbits, sg);
                old[e] = __builtin_nan("");
            }
            plane_load4(p_min + at, old, c0, left, right);
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) x[e] = fmin(old[e], x[e]);
            plane_store4(p_min + at, x, c0, left, right);
        }
        if constexpr ((LIVE & RA_MAX) != 0) {
            double x[4], old[4];
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                x[e] = leaf_extreme(hi[a][e], INT32_MIN, enc, fbits, sg);
                old[e] = __builtin_nan("");
            }
            plane_load4(p_max + at, old, c0, left, right);
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) x[e] = fmax(old[e], x[e]);
            plane_store4(p_max + at, x, c0, left, right);
        }
    }
}
// k_bulk_reduce with a label per instant (labels[U.lab + (t - U.t0)], uniform over the workgroup, read once per instant): the
// register accumulators hold one run of equal labels.  On a change of group -- and, through the same code, behind the last
// instant -- the run is merged into its group's planes (group_merge16); a new run starts from the identities and its group's
// running SUM.  A thread always meets the same cells, so what it stored for a group it loads back itself when the group returns.
// Instants of no group are neither decoded nor merged: every instant is decoded from its block's Snapshot and its own Log alone
// (bulk_instant keeps track of the Snapshot in the pyramid).
template <uint32_t LIVE>
__global__ void __launch_bounds__(256)
k_bulk_group(const ChunkRef* __restrict__ chunks, const uint8_t* __restrict__ encs, const GroupUnit* __restrict__ units, uint32_t n_units,
             const uint16_t* __restrict__ labels, uint32_t n_groups, double* dst, double* scr, uint32_t ops) {
    typedef int32_t V;
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t END = 0xffffffffu;  // the "label" behind the unit's last instant: it differs from every group
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const GroupUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const int32_t enc = (int32_t)encs[U.chunk];
        const int kind = leaf_kind(enc);
        const int64_t div = (int64_t)1 << (C.fbits + 1u);  // from_fixed's divisor
        const double inv = 1.0 / (double)div;
        const float invf = 1.0f / (float)div;
        const int32_t sg = leaf_mirror(kind, C.fbits);
        const gbytes gb = (gbytes)C.bytes;
        const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
        // group 0's planes; group g's are g * U.gsz on
        double* const p_min = reduce_plane(RA_MIN, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_max = reduce_plane(RA_MAX, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_sum = reduce_plane(RA_SUM, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_cnt = reduce_plane(RA_COUNT, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double sum[4][4];
        uint32_t cnt[4][4];
        int32_t lo[4][4], hi[4][4];
        uint32_t cur = GROUP_NONE, run = 0;  // the open run's group and length
        uint32_t cur_snap = 0xffffffffu;
        for (uint32_t t = U.t0;; t++) {
            const uint32_t lab = t < U.t1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)labels[U.lab + (t - U.t0)]) : END;
            if (lab != END && lab >= n_groups) continue;
            if (lab != cur) {
                if (cur != GROUP_NONE) {
                    const uint64_t go = (uint64_t)cur * U.gsz;
                    group_merge16<LIVE>(U, tid, kind, enc, C.fbits, sg, run, p_min + go, p_max + go, p_sum + go, p_cnt + go, sum, cnt, lo, hi);
                }
                if (lab == END) break;
                cur = lab;
                run = 0;
                uint32_t tl = tid;  // (as in group_merge16: the places of the cells are not kept over the walk)
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (uint32_t a = 0; a < 4u; a++) {
#pragma unroll
                    for (uint32_t e = 0; e < 4u; e++) {
                        sum[a][e] = 0.0;
                        cnt[a][e] = 0u;
                        lo[a][e] = INT32_MAX;
                        hi[a][e] = INT32_MIN;
                    }
                    if constexpr ((LIVE & RA_SUM) != 0) {
                        const uint32_t g = tl + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
                        if (r >= top && r < bottom && c0 + 4u > left && c0 < right)
                            plane_load4(p_sum + (uint64_t)cur * U.gsz + ((int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left)), sum[a], c0, left, right);
                    }
                }
            }
            run++;
            const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                const uint32_t r0 = (uint32_t)U.rr + 2u * rp, c0 = (uint32_t)U.rc + 4u * cg;  // chunk coordinates
                if (r0 + 2u <= top || r0 >= bottom || c0 + 4u <= left || c0 >= right) continue;
                V v[2][4];
                bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                for (uint32_t i = 0; i < 2u; i++) {
                    const uint32_t r = r0 + i, a = 2u * k + i;
                    if (r < top || r >= bottom) continue;
                    if (kind == 0) reduce_fold4<LIVE, 0>(v[i], sum[a], cnt[a], lo[a], hi[a], inv, invf, sg);
                    else if (kind == 1) reduce_fold4<LIVE, 1>(v[i], sum[a], cnt[a], lo[a], hi[a], inv, invf, sg);
                    else reduce_fold4<LIVE, 2>(v[i], sum[a], cnt[a], lo[a], hi[a], inv, invf, sg);
                }
            }
        }
        __syncthreads();
    }
}

int launch_bulk_group(const ChunkRef* d_refs, const uint8_t* d_enc, const GroupUnit* d_units, uint32_t n, const uint16_t* d_labels,
                      uint32_t n_groups, double* d_dst, double* d_scr, uint32_t ops) {
    if (n == 0) return DCDF_OK;
    const dim3 grid = bulk_grid(n), block(256);
#define K2R_GROUP_CASE(L) \
    case L: hipLaunchKernelGGL((k_bulk_group<L>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_labels, n_groups, d_dst, d_scr, ops); break;
    switch (reduce_live(ops)) {
        K2R_GROUP_CASE(1) K2R_GROUP_CASE(2) K2R_GROUP_CASE(3) K2R_GROUP_CASE(4) K2R_GROUP_CASE(5)
        K2R_GROUP_CASE(6) K2R_GROUP_CASE(7) K2R_GROUP_CASE(8) K2R_GROUP_CASE(9) K2R_GROUP_CASE(10)
        K2R_GROUP_CASE(11) K2R_GROUP_CASE(12) K2R_GROUP_CASE(13) K2R_GROUP_CASE(14) K2R_GROUP_CASE(15)
        default: return DCDF_ERR_BAD_ARG;
    }
#undef K2R_GROUP_CASE
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- moments over time (k2r_moment.h): the state (c, K, s1, s2) of one run of equal labels at a time ---------------------------
// The thread's 16 states from (STORE false) or into (STORE true) the planes of one group (p_*: already moved to that group),
// whole: there is no merge rule.  The count is kept as an integer -- it never exceeds the instants of a cube -- and converts to
// the double the planes hold.  As in group_merge16, the cells' places are worked out again at every call.
template <bool STORE>
__device__ __forceinline__ void moment_state16(const GroupUnit& U, uint32_t tid, double* p_c, double* p_k, double* p_s1, double* p_s2,
                                               uint32_t (&cnt)[4][4], double (&K)[4][4], double (&s1)[4][4], double (&s2)[4][4]) {
    const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (uint32_t a = 0; a < 4u; a++) {
        double x[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            x[e] = STORE ? (double)cnt[a][e] : 0.0;
            if constexpr (!STORE) {  // (the identities: cells outside the unit's rectangle are neither folded nor stored)
                K[a][e] = __builtin_nan("");
                s1[a][e] = 0.0;
                s2[a][e] = 0.0;
            }
        }
        const uint32_t g = tid + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
        if (r >= top && r < bottom && c0 + 4u > left && c0 < right) {
            const int64_t at = (int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left);
            if constexpr (STORE) {
                plane_store4(p_c + at, x, c0, left, right);
                plane_store4(p_k + at, K[a], c0, left, right);
                plane_store4(p_s1 + at, s1[a], c0, left, right);
                plane_store4(p_s2 + at, s2[a], c0, left, right);
            } else {
                plane_load4(p_c + at, x, c0, left, right);
                plane_load4(p_k + at, K[a], c0, left, right);
                plane_load4(p_s1 + at, s1[a], c0, left, right);
                plane_load4(p_s2 + at, s2[a], c0, left, right);
            }
        }
        if constexpr (!STORE) {
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) cnt[a][e] = (uint32_t)x[e];
        }
    }
}
// One instant of four cells into their states: reduce_fold4's value conversions by kind (x has from_fixed's bits; a float leaf's
// stored 0 is NaN), then the contract's step.  Only x depends on the kind -- a uniform branch --; the states are updated by one
// piece of code for all three.  With a state update per kind the registers of the 16 states were copied at every join: 350
// VGPRs + AGPRs, one wave per SIMD, against 212 this way.
__device__ __forceinline__ void moment_fold4(int kind, const int32_t (&v)[4], uint32_t (&cnt)[4], double (&K)[4], double (&s1)[4], double (&s2)[4], double inv,
                                             float invf) {
#pragma clang fp contract(off)
    double x[4];
    if (kind == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) x[e] = (double)v[e];
    } else if (kind == 1) {
#pragma unroll
        for (int e = 0; e < 4; e++) x[e] = v[e] != 0 ? (double)((float)(v[e] - 1) * invf) : __builtin_nan("");
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) x[e] = v[e] != 0 ? (double)(v[e] - 1) * inv : __builtin_nan("");
    }
#pragma unroll
    for (int e = 0; e < 4; e++) moment_step(cnt[e], K[e], s1[e], s2[e], x[e]);
}
// k_bulk_group's walk with the moments' state: labels[U.lab + (t - U.t0)] per instant, or group 0 throughout without a label
// array.  The instants are taken a run of equal labels at a time: the run's group's state is loaded whole, the run's instants
// are folded in an inner loop, the state is stored whole -- the planes were filled with the identities before the first
// segment, so a group's first touch is a load like any other, and a thread always meets the same cells.  Instants of no group
// are not decoded and end no run.  (Loading and storing inside one loop over the instants, as k_bulk_group merges, kept two
// copies of the states in registers.)  One instantiation: `ops` only decides which planes are output and which scratch
// (moment_plane).
__global__ void __launch_bounds__(256)
k_bulk_moment(const ChunkRef* __restrict__ chunks, const uint8_t* __restrict__ encs, const GroupUnit* __restrict__ units, uint32_t n_units,
              const uint16_t* __restrict__ labels, uint32_t n_groups, double* dst, double* scr, uint32_t ops) {
    typedef int32_t V;
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t END = 0xffffffffu;  // the "label" behind the unit's last instant: it differs from every group
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const GroupUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const int kind = leaf_kind((int32_t)encs[U.chunk]);
        const int64_t div = (int64_t)1 << (C.fbits + 1u);  // from_fixed's divisor
        const double inv = 1.0 / (double)div;
        const float invf = 1.0f / (float)div;
        const gbytes gb = (gbytes)C.bytes;
        const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
        // group 0's planes; group g's are g * U.gsz on
        double* const p_c = moment_plane(MS_COUNT, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_k = moment_plane(MS_K, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_s1 = moment_plane(MS_S1, dst, scr, ops, U.o_off, U.s_off, U.psz);
        double* const p_s2 = moment_plane(MS_S2, dst, scr, ops, U.o_off, U.s_off, U.psz);
        uint32_t cnt[4][4];
        double K[4][4], s1[4][4], s2[4][4];
        uint32_t cur_snap = 0xffffffffu;
        uint32_t t = U.t0;
        for (;;) {
            uint32_t lab = END;
            for (; t < U.t1; t++) {
                lab = labels ? (uint32_t)__builtin_amdgcn_readfirstlane((int)labels[U.lab + (t - U.t0)]) : 0u;
                if (lab < n_groups) break;
            }
            if (t >= U.t1) break;
            const uint64_t go = (uint64_t)lab * U.gsz;
            moment_state16<false>(U, tid, p_c + go, p_k + go, p_s1 + go, p_s2 + go, cnt, K, s1, s2);
            for (;;) {
                const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
#pragma unroll
                for (uint32_t k = 0; k < 2u; k++) {
                    const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                    const uint32_t r0 = (uint32_t)U.rr + 2u * rp, c0 = (uint32_t)U.rc + 4u * cg;  // chunk coordinates
                    if (r0 + 2u <= top || r0 >= bottom || c0 + 4u <= left || c0 >= right) continue;
                    V v[2][4];
                    bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                    for (uint32_t i = 0; i < 2u; i++) {
                        const uint32_t r = r0 + i, a = 2u * k + i;
                        if (r < top || r >= bottom) continue;
                        moment_fold4(kind, v[i], cnt[a], K[a], s1[a], s2[a], inv, invf);
                    }
                }
                uint32_t next = END;
                for (t++; t < U.t1; t++) {
                    next = labels ? (uint32_t)__builtin_amdgcn_readfirstlane((int)labels[U.lab + (t - U.t0)]) : 0u;
                    if (next < n_groups) break;
                }
                if (t >= U.t1 || next != lab) break;
            }
            moment_state16<true>(U, tid, p_c + go, p_k + go, p_s1 + go, p_s2 + go, cnt, K, s1, s2);
        }
        __syncthreads();
    }
}

int launch_bulk_moment(const ChunkRef* d_refs, const uint8_t* d_enc, const GroupUnit* d_units, uint32_t n, const uint16_t* d_labels,
                       uint32_t n_groups, double* d_dst, double* d_scr, uint32_t ops) {
    if (n == 0) return DCDF_OK;
    if (ops == 0 || ops > MO_ALL) return DCDF_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_bulk_moment, bulk_grid(n), dim3(256), 0, 0, d_refs, d_enc, d_units, n, d_labels, n_groups, d_dst, d_scr, ops);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- reduction over space (k2r_space.h): the walk's cells into one record per instant --------------------------------------
// One instant of one selected cell into the thread's four values.  kind as in k_bulk_reduce (uniform over a unit).  m is the
// integer the decoder divides (space_m): n itself, (float)(n - 1) -- which rounds beyond 2^24 -- or n - 1; |m| <= 2^30 here, so a
// unit's 4096 cells stay below 2^43 in an int64.  lo / hi hold the extremes as stored integers, mirrored by sg (reduce_fold4's
// monotonicity argument).
template <uint32_t LIVE>
__device__ __forceinline__ void space_fold1(int32_t n, bool sel, int kind, int64_t& s, uint32_t& cnt, int32_t& lo, int32_t& hi, int32_t sg) {
    const bool ok = sel && (kind == 0 || n != 0);
    if constexpr ((LIVE & RA_SUM) != 0) {
        const int32_t d = n - (kind != 0 ? 1 : 0);
        const int32_t m = kind == 1 ? (int32_t)(float)d : d;
        s += ok ? (int64_t)m : (int64_t)0;
    }
    if constexpr ((LIVE & RA_COUNT) != 0) cnt += ok ? 1u : 0u;
    const int32_t key = (n ^ sg) - sg;
    if constexpr ((LIVE & RA_MIN) != 0) lo = ok && key < lo ? key : lo;
    if constexpr ((LIVE & RA_MAX) != 0) hi = ok && key > hi ? key : hi;
}

constexpr uint32_t SPACE_B = 16;  // instants whose wave results wait in LDS before one barrier flushes them

// LIVE: the values this instantiation carries (RA_*; MIN and MAX go together, SUM and COUNT go together).  MASKED: the cube has
// a mask.  Which of a thread's 16 cells count -- inside the unit's rectangle, and their mask byte non-zero -- is one 16-bit
// word per unit (bulk_select16), never looked up per instant.  Per instant the thread folds its cells, the wave folds its
// lanes (__shfl_xor), and lane 0 leaves the wave's result in the instant's LDS slot; every SPACE_B instants one barrier lets
// SPACE_B threads fold the four waves and write the records.
// (waves_per_eu: the allocator stays within 128 VGPRs -- k_bulk_decode's four waves per SIMD -- instead of 133-135; no scratch.)
template <uint32_t LIVE, bool MASKED>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_bulk_space(const ChunkRef* __restrict__ chunks, const uint8_t* __restrict__ encs, const SpaceUnit* __restrict__ units, uint32_t n_units,
             const uint8_t* __restrict__ mask, SpacePartial* __restrict__ recs) {
    typedef int32_t V;
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    __shared__ int64_t w_sum[SPACE_B][4];
    __shared__ uint32_t w_cnt[SPACE_B][4];
    __shared__ int32_t w_lo[SPACE_B][4], w_hi[SPACE_B][4];
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const SpaceUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const int32_t enc = (int32_t)encs[U.chunk];
        const int kind = leaf_kind(enc);
        const int32_t sg = leaf_mirror(kind, C.fbits);
        const gbytes gb = (gbytes)C.bytes;
        const uint32_t sel = bulk_select16<MASKED>(U, mask, tid);  // the thread's cells that count
        uint32_t cur_snap = 0xffffffffu;
        for (uint32_t t = U.t0; t < U.t1; t++) {
            const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
            // ---- nodes of side 2, two per task: their 2 x 4 cells, folded ----
            int64_t s = 0;
            uint32_t cnt = 0;
            int32_t lo = INT32_MAX, hi = INT32_MIN;  // (beyond every stored value of a narrow32 chunk: "no value yet")
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                const uint32_t sel8 = (sel >> (8u * k)) & 255u;
                if (sel8 == 0) continue;  // (none of the group's cells counts)
                V v[2][4];
                bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                for (uint32_t i = 0; i < 2u; i++)
#pragma unroll
                    for (uint32_t c = 0; c < 4u; c++) {
                        const bool on = ((sel8 >> (4u * i + c)) & 1u) != 0;
                        space_fold1<LIVE>(v[i][c], on, kind, s, cnt, lo, hi, sg);
                    }
            }
            // ---- the wave's lanes, then its slot ----
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                if constexpr ((LIVE & RA_SUM) != 0) s += __shfl_xor((long long)s, off);
                if constexpr ((LIVE & RA_COUNT) != 0) cnt += __shfl_xor(cnt, off);
                if constexpr ((LIVE & RA_MIN) != 0) lo = min(lo, __shfl_xor(lo, off));
                if constexpr ((LIVE & RA_MAX) != 0) hi = max(hi, __shfl_xor(hi, off));
            }
            const uint32_t slot = (t - U.t0) % SPACE_B;
            if ((tid & 63u) == 0) {
                w_sum[slot][tid >> 6] = s;
                w_cnt[slot][tid >> 6] = cnt;
                w_lo[slot][tid >> 6] = lo;
                w_hi[slot][tid >> 6] = hi;
            }
            if (slot == SPACE_B - 1u || t + 1u == U.t1) {  // the slots 0 .. slot hold the instants t - slot .. t
                __syncthreads();
                if (tid <= slot) {
                    int64_t ts = 0;
                    uint32_t tc = 0;
                    int32_t tl = INT32_MAX, th = INT32_MIN;
#pragma unroll
                    for (uint32_t w = 0; w < 4u; w++) {
                        ts += w_sum[tid][w];
                        tc += w_cnt[tid][w];
                        tl = min(tl, w_lo[tid][w]);
                        th = max(th, w_hi[tid][w]);
                    }
                    __attribute__((address_space(1))) SpacePartial* const o =
                        (__attribute__((address_space(1))) SpacePartial*)recs + (U.rec + (uint64_t)(t - U.t0 - slot + tid));
                    o->hi = ts < 0 ? ~(uint64_t)0 : (uint64_t)0;
                    o->lo = (uint64_t)ts;
                    o->mn = leaf_extreme(tl, INT32_MAX, enc, C.fbits, sg);
                    o->mx = leaf_extreme(th, INT32_MIN, enc, C.fbits, sg);
                    o->cnt = tc;
                    o->scale = space_scale(enc, C.fbits);
                }
            }
        }
        __syncthreads();
    }
}

int launch_bulk_space(const ChunkRef* d_refs, const uint8_t* d_enc, const SpaceUnit* d_units, uint32_t n, const uint8_t* d_mask,
                      SpacePartial* d_recs, uint32_t live) {
    if (n == 0) return DCDF_OK;
    const dim3 grid = bulk_grid(n), block(256);
    constexpr uint32_t EXT = RA_MIN | RA_MAX, ADD = RA_SUM | RA_COUNT;
    const uint32_t l = ((live & EXT) ? EXT : 0u) | ((live & ADD) ? ADD : 0u);
#define K2R_SPACE_CASE(L)                                                                                                          \
    case L:                                                                                                                        \
        if (d_mask) hipLaunchKernelGGL((k_bulk_space<L, true>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_mask, d_recs);       \
        else hipLaunchKernelGGL((k_bulk_space<L, false>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_mask, d_recs);             \
        break;
    switch (l) {
        K2R_SPACE_CASE(EXT) K2R_SPACE_CASE(ADD) K2R_SPACE_CASE(EXT | ADD)
        default: return DCDF_ERR_BAD_ARG;
    }
#undef K2R_SPACE_CASE
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- value histograms (k2r_hist.h): the walk's cells into counts per instant and bin ----------------------------------------
// K2R_HIST_VARIANT (diagnostic builds for DESIGN.md section 4h only, tools/build_variant.sh; their counts are wrong on purpose):
// 1 = the binning compiled out (no threshold search: every cell goes to the first bin), 2 = the LDS and global adds compiled out
// (the bins are searched and folded into a register), 3 = the 16 searches of a thread one after the other instead of 8 in step.
#ifndef K2R_HIST_VARIANT
#define K2R_HIST_VARIANT 0
#endif
constexpr uint32_t HIST_SLOTS = 16;     // instants whose counts wait in LDS before one barrier flushes them, at most
constexpr uint32_t HIST_COUNTS = 1024;  // LDS counters: min(HIST_SLOTS, HIST_COUNTS / n_bins) instants of n_bins (4 at 256 bins)
constexpr uint32_t HIST_THR = 512;      // entries of the largest threshold table (hist_steps(256) = 9)

// MASKED: the cube has a mask.  A thread owns its 16 cells of the walk and bulk_select16's word of those that count.  The unit's
// leaf has one table of int32 thresholds (hist_thresholds32, made by the planner once per distinct encoding and fractional
// bits), copied to LDS before the first instant; a cell's bin is a branch-free binary search of `steps` LDS reads -- integer
// compares only, nothing is widened.  The searches of a group's 8 cells advance together, step by step: a search is a chain of
// dependent LDS reads, and 8 independent chains hide each other's latency (0.5 ms of 5.8 at 16 bins on the benchmark cube,
// DESIGN.md section 4h).  The NaN code of a float leaf and cells outside the edges are dropped.
//
// Smooth data puts most of a wave's cells into one bin.  A thread therefore adds a RUN of equal bins among its cells with one
// LDS atomic; on a constant field that is one add per thread and instant.  (Combining the lanes' last runs across the wave
// first -- ballot, the first pending lane's bin, a __shfl_xor sum, one add -- was built and measured: no faster on a constant
// field, 3 % slower on real data)
//
// Every `slots` instants (or at the unit's end) one barrier lets the workgroup add the non-zero counters to the cube's rows --
// device-scope 64-bit atomic adds, contiguous over (instant, bin) -- and clear them; the barrier bulk_instant begins the next
// instant with puts the clears before its adds.  (waves_per_eu: k_bulk_space's reason; no scratch.)
template <bool MASKED>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_bulk_hist(const ChunkRef* __restrict__ chunks, const uint8_t* __restrict__ encs, const HistUnit* __restrict__ units, uint32_t n_units,
            const uint8_t* __restrict__ mask, const int32_t* __restrict__ thr, uint32_t n_bins, uint32_t steps, uint64_t* out) {
    typedef int32_t V;
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    __shared__ int32_t s_thr[HIST_THR];
    __shared__ uint32_t s_cnt[HIST_COUNTS];
    const uint32_t tid = threadIdx.x;
    const uint32_t fit = HIST_COUNTS / n_bins, slots = fit < HIST_SLOTS ? fit : HIST_SLOTS;
    for (uint32_t i = tid; i < HIST_COUNTS; i += 256u) s_cnt[i] = 0u;  // (every flush leaves them cleared)
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const HistUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const int32_t enc = (int32_t)encs[U.chunk];
        const bool is_float = leaf_kind(enc) != 0;
        const gbytes gb = (gbytes)C.bytes;
        // the leaf's thresholds (read after the first instant's barriers; the previous unit's readers are behind its last barrier)
        for (uint32_t i = tid; i < ((uint32_t)1 << steps); i += 256u)
            s_thr[i] = ((const __attribute__((address_space(1))) int32_t*)thr)[U.thr + i];
        const uint32_t sel = bulk_select16<MASKED>(U, mask, tid);  // the thread's cells that count
        uint32_t cur_snap = 0xffffffffu, slot = 0;
        for (uint32_t t = U.t0; t < U.t1; t++) {
            const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
            // ---- nodes of side 2, two per task: their 2 x 4 cells, binned ----
            uint32_t* const row = s_cnt + slot * n_bins;
            uint32_t run_bin = 0, run = 0;  // the thread's current run of equal bins
#if K2R_HIST_VARIANT == 2
            uint32_t sink = row[0];
#define K2R_HIST_ADD(b, c) sink = sink * 31u + (b) + (c)
#else
#define K2R_HIST_ADD(b, c) atomicAdd(row + (b), (c))
#endif
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                const uint32_t sel8 = (sel >> (8u * k)) & 255u;
                if (sel8 == 0) continue;  // (none of the group's cells counts)
                V v[2][4];
                bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
                uint32_t pos[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // hist_search32, the 8 searches in step
#if K2R_HIST_VARIANT == 1
#pragma unroll
                for (uint32_t e = 0; e < 8u; e++) pos[e] = v[e >> 2][e & 3u] == INT32_MIN ? 0u : 1u;
#elif K2R_HIST_VARIANT == 3
#pragma unroll
                for (uint32_t e = 0; e < 8u; e++) pos[e] = (uint32_t)(hist_search32(s_thr, steps, v[e >> 2][e & 3u]) + 1);
#else
                for (uint32_t s = (uint32_t)1 << (steps - 1u); s; s >>= 1) {
#pragma unroll
                    for (uint32_t e = 0; e < 8u; e++) pos[e] += s_thr[pos[e] + s - 1u] <= v[e >> 2][e & 3u] ? s : 0u;
                }
#endif
#pragma unroll
                for (uint32_t e = 0; e < 8u; e++) {
                    const uint32_t p = pos[e] - 1u;  // (0 - 1 wraps beyond n_bins)
                    const bool on = ((sel8 >> e) & 1u) != 0 && !(is_float && v[e >> 2][e & 3u] == 0) && p < n_bins;
                    const uint32_t bin = U.rev ? n_bins - 1u - p : p;
                    if (on) {
                        if (run != 0 && bin != run_bin) {
                            K2R_HIST_ADD(run_bin, run);
                            run = 0;
                        }
                        run_bin = bin;
                        run += 1u;
                    }
                }
            }
            if (run != 0) K2R_HIST_ADD(run_bin, run);  // the thread's last run
#if K2R_HIST_VARIANT == 2
            if (sink == 0xdeadbeefu && t + 1u == U.t1) out[U.o_off] = sink;  // (keeps the searches alive; never true in practice)
            continue;
#endif
            // ---- the slots' counters into the cube's rows ----
            if (slot + 1u == slots || t + 1u == U.t1) {  // the slots 0 .. slot hold the instants t - slot .. t
                __syncthreads();
                __attribute__((address_space(1))) unsigned long long* const o =
                    (__attribute__((address_space(1))) unsigned long long*)out + (U.o_off + (uint64_t)(t - U.t0 - slot) * n_bins);
                for (uint32_t i = tid; i < (slot + 1u) * n_bins; i += 256u) {
                    const uint32_t c = s_cnt[i];
                    if (c != 0) {
                        s_cnt[i] = 0u;
                        __hip_atomic_fetch_add(o + i, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                slot = 0;
            } else {
                slot += 1u;
            }
        }
        __syncthreads();
    }
}

#undef K2R_HIST_ADD

int launch_bulk_hist(const ChunkRef* d_refs, const uint8_t* d_enc, const HistUnit* d_units, uint32_t n, const uint8_t* d_mask,
                     const int32_t* d_thr, uint32_t n_bins, uint64_t* d_out) {
    if (n == 0) return DCDF_OK;
    if (n_bins == 0 || n_bins > HIST_MAX_BINS) return DCDF_ERR_BAD_ARG;
    static_assert(((uint32_t)1 << 9) == HIST_THR && HIST_MAX_BINS + 2u <= HIST_THR, "the largest table fits s_thr");
    static_assert(HIST_COUNTS >= HIST_MAX_BINS, "one instant's counters fit s_cnt");
    const dim3 grid = bulk_grid(n), block(256);
    const uint32_t steps = hist_steps(n_bins);
    if (d_mask) hipLaunchKernelGGL((k_bulk_hist<true>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_mask, d_thr, n_bins, steps, d_out);
    else hipLaunchKernelGGL((k_bulk_hist<false>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_mask, d_thr, n_bins, steps, d_out);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- zonal statistics (k2r_zonal.h): the walk's cells into one accumulator entry per (zone, instant) -----------------------
// The label of the thread's cell b (bulk_select16's numbering and addresses, 2-byte elements): ZONAL_NONE outside the unit's
// rectangle or for a label that names no zone.
__device__ __forceinline__ uint32_t zonal_label(const ZonalUnit& U, const uint16_t* labels, uint32_t n_zones, uint32_t tid, uint32_t b) {
    const uint32_t g = tid + 256u * (b >> 3), r = (uint32_t)U.rr + 2u * (g >> 4) + ((b >> 2) & 1u), c = (uint32_t)U.rc + 4u * (g & 15u) + (b & 3u);
    if (!(r >= U.top && r < U.bottom && c >= U.left && c < U.right)) return ZONAL_NONE;
    const uint32_t l = ((const __attribute__((address_space(1))) uint16_t*)labels)[U.m_off + (uint64_t)(r - U.top) * U.m_sr + (c - U.left)];
    return l < n_zones ? l : ZONAL_NONE;
}

// LIVE: the values this instantiation carries (k_bulk_space's groups: MIN and MAX go together, SUM and COUNT go together; the
// count is always kept, it says which entries hold anything).  A unit has one leaf, so inside it the sums are int64 sums of m and
// the extremes mirrored int32 keys, as in k_bulk_space; what differs is where a cell's value goes.
//
// Per unit: the distinct labels of its selected cells are ranked -- a bitmap of 65536 bits in the first 8 KB of `pyr`, which is
// dead until bulk_instant refills it, and a popcount scan behind it (zonal_rank; the scan's counts pass through `nst`) -- and the labels of the ranks [r0, r0 + ZONAL_ZL)
// get the zone slots of this round: the list in LDS, each cell's slot in 4 bits of a register pair.  A unit with more distinct labels
// walks its instants again for the next ZONAL_ZL ranks (rare: a unit is 64 x 64 cells of one zone, or of a few).  A unit whose
// selected cells all carry one label skips the ranking (a min / max over the workgroup says so).
//
// Per instant: a unit of one zone folds as k_bulk_space does -- the thread's cells, the wave's lanes by __shfl_xor, one LDS
// update per wave; otherwise a thread adds every RUN of equal slots among its 16 cells to the LDS accumulators of (instant slot,
// zone slot) with LDS atomics (k_bulk_hist's run trick).  Every ZONAL_B instants, or at the round's end, one barrier lets the
// workgroup add the entries that hold anything to the global accumulators (zonal_add) and clear them.
// (waves_per_eu: k_bulk_space's reason; no scratch.)
struct ZonalLds {  // one LDS accumulator: a unit's share of one (instant, zone), in the leaf's own integers
    unsigned long long sum;
    uint32_t cnt;
    int32_t lo, hi;
    uint32_t _pad;
};
template <uint32_t LIVE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_bulk_zonal(const ChunkRef* __restrict__ chunks, const uint8_t* __restrict__ encs, const ZonalUnit* __restrict__ units, uint32_t n_units,
             const uint16_t* __restrict__ labels, uint32_t n_zones, uint64_t* acc) {
    typedef int32_t V;
    constexpr uint32_t L1 = LIVE | RA_COUNT, NE = ZONAL_B * ZONAL_ZL;
    constexpr bool EXT = (LIVE & (RA_MIN | RA_MAX)) != 0, ADD = (LIVE & RA_SUM) != 0;
    static_assert(2u * ZONAL_BM_WORDS <= BP_SIZE, "the bitmap and its prefix counts fit the pyramid's array");
    static_assert(ZONAL_ZL == 16, "a cell's slot is 4 bits");
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    __shared__ ZonalLds za[NE];  // [instant slot][zone slot]
    __shared__ uint32_t zlist[ZONAL_ZL];
    __shared__ uint32_t w_lo[4], w_hi[4];
    const uint32_t tid = threadIdx.x;
    uint32_t* const bm = (uint32_t*)pyr;
    uint32_t* const pre = bm + ZONAL_BM_WORDS;
    for (uint32_t i = tid; i < NE; i += 256u) za[i] = ZonalLds{0, 0u, INT32_MAX, INT32_MIN, 0u};  // (every flush leaves them so)
    // One loop over (unit, round): the unit is read again for every round, so nothing of its label addresses outlives the ranking.
    for (uint32_t u = blockIdx.x, r0 = 0; u < n_units;) {
        const ZonalUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const int32_t enc = (int32_t)encs[U.chunk];
        const int kind = leaf_kind(enc);
        const int32_t sg = leaf_mirror(kind, C.fbits);
        const gbytes gb = (gbytes)C.bytes;
        uint32_t n_distinct = 1;
        {
            // ---- the round's zone slots: sel = the thread's cells that count now, zs = their slots, 4 bits each ----
            uint32_t sel = 0;
            uint64_t zs = 0;
            uint32_t lmin = ZONAL_NONE, lmax = 0;
            uint32_t lab[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the labels of the thread's cells, two to a register; dead after the ranking
#define K2R_ZONAL_LAB(b) ((lab[(b) >> 1] >> (16u * ((b) & 1u))) & 0xffffu)
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++) {
                const uint32_t l = zonal_label(U, labels, n_zones, tid, b);
                lab[b >> 1] |= l << (16u * (b & 1u));
                if (l != ZONAL_NONE) {
                    lmin = min(lmin, l);
                    lmax = max(lmax, l);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lmin = min(lmin, __shfl_xor(lmin, off));
                lmax = max(lmax, __shfl_xor(lmax, off));
            }
            if ((tid & 63u) == 0) {
                w_lo[tid >> 6] = lmin;
                w_hi[tid >> 6] = lmax;
            }
            __syncthreads();  // (also: the previous round's and unit's readers of pyr and zlist are done)
            lmin = min(min(w_lo[0], w_lo[1]), min(w_lo[2], w_lo[3]));
            lmax = max(max(w_hi[0], w_hi[1]), max(w_hi[2], w_hi[3]));
            const bool any = lmin != ZONAL_NONE;  // a cell of the unit is in a zone (uniform: every thread read the same words)
            const bool one = lmin == lmax;
            if (!any) {
                n_distinct = 0;
            } else if (one) {
                if (tid == 0) zlist[0] = lmin;
#pragma unroll
                for (uint32_t b = 0; b < 16u; b++) sel |= K2R_ZONAL_LAB(b) == lmin ? 1u << b : 0u;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 8u; j++) bm[8u * tid + j] = 0u;
                __syncthreads();
                uint32_t prev = ZONAL_NONE;
#pragma unroll
                for (uint32_t b = 0; b < 16u; b++) {
                    const uint32_t l = K2R_ZONAL_LAB(b);
                    if (l != ZONAL_NONE && l != prev) atomicOr(bm + (l >> 5), 1u << (l & 31u));
                    prev = l;
                }
                __syncthreads();
                // the exclusive scan of the threads' counts, through `nst` (dead like `pyr`): groups of 16, then the groups' totals
                const uint32_t mine = zonal_count8(bm, tid);
                nst[tid] = mine;
                __syncthreads();
                if (tid < 16u) {
                    uint32_t run = 0;
                    for (uint32_t j = 0; j < 16u; j++) {
                        const uint32_t c = nst[16u * tid + j];
                        nst[16u * tid + j] = run;
                        run += c;
                    }
                    nst[256u + tid] = run;
                }
                __syncthreads();
                uint32_t start = nst[tid], total = 0;
                for (uint32_t g = 0; g < 16u; g++) {
                    const uint32_t c = nst[256u + g];
                    start += g < (tid >> 4) ? c : 0u;
                    total += c;
                }
                n_distinct = total;
                zonal_prefix8(bm, pre, tid, start);
                __syncthreads();
#pragma unroll
                for (uint32_t b = 0; b < 16u; b++) {
                    const uint32_t l = K2R_ZONAL_LAB(b);
                    if (l == ZONAL_NONE) continue;
                    const uint32_t s = zonal_rank(bm, pre, l) - r0;  // (wraps beyond ZONAL_ZL below r0)
                    if (s < ZONAL_ZL) {
                        sel |= 1u << b;
                        zs |= (uint64_t)s << (4u * b);
                        zlist[s] = l;  // (every writer of a slot writes its one label)
                    }
                }
            }
            // ---- the unit's instants ----
            uint32_t cur_snap = 0xffffffffu, slot = 0;
            for (uint32_t t = U.t0; any && t < U.t1; t++) {
                const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
                const uint32_t row = slot * ZONAL_ZL;
                int64_t s = 0;
                uint32_t cnt = 0;
                int32_t lo = INT32_MAX, hi = INT32_MIN;  // (beyond every stored value of a narrow32 chunk: "no value yet")
#define K2R_ZONAL_PUT(at)                                                              \
    {                                                                                  \
        ZonalLds* const za_e = za + (at);                                              \
        if constexpr (ADD) atomicAdd(&za_e->sum, (unsigned long long)s);               \
        atomicAdd(&za_e->cnt, cnt);                                                    \
        if constexpr (EXT) {                                                           \
            atomicMin(&za_e->lo, lo);                                                  \
            atomicMax(&za_e->hi, hi);                                                  \
        }                                                                              \
    }
                if (one) {
#pragma unroll
                    for (uint32_t k = 0; k < 2u; k++) {
                        const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                        const uint32_t sel8 = (sel >> (8u * k)) & 255u;
                        if (sel8 == 0) continue;  // (none of the group's cells counts)
                        V v[2][4];
                        bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                        for (uint32_t i = 0; i < 2u; i++)
#pragma unroll
                            for (uint32_t c = 0; c < 4u; c++) space_fold1<L1>(v[i][c], ((sel8 >> (4u * i + c)) & 1u) != 0, kind, s, cnt, lo, hi, sg);
                    }
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        if constexpr (ADD) s += __shfl_xor((long long)s, off);
                        cnt += __shfl_xor(cnt, off);
                        if constexpr (EXT) {
                            lo = min(lo, __shfl_xor(lo, off));
                            hi = max(hi, __shfl_xor(hi, off));
                        }
                    }
                    if ((tid & 63u) == 0 && cnt != 0) K2R_ZONAL_PUT(row)
                } else {
                    uint32_t run_slot = 0;  // the thread's current run of equal slots: cnt != 0 while it holds anything
#pragma unroll
                    for (uint32_t k = 0; k < 2u; k++) {
                        const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                        const uint32_t sel8 = (sel >> (8u * k)) & 255u;
                        if (sel8 == 0) continue;
                        V v[2][4];
                        bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                        for (uint32_t j = 0; j < 8u; j++) {
                            const int32_t n = v[j >> 2][j & 3u];
                            const bool on = ((sel8 >> j) & 1u) != 0 && (kind == 0 || n != 0);
                            const uint32_t zslot = (uint32_t)(zs >> (4u * (8u * k + j))) & 15u;
                            if (on) {
                                if (cnt != 0 && zslot != run_slot) {
                                    K2R_ZONAL_PUT(row + run_slot)
                                    s = 0;
                                    cnt = 0;
                                    lo = INT32_MAX;
                                    hi = INT32_MIN;
                                }
                                run_slot = zslot;
                                space_fold1<L1>(n, true, kind, s, cnt, lo, hi, sg);
                            }
                        }
                    }
                    if (cnt != 0) K2R_ZONAL_PUT(row + run_slot)  // the thread's last run
                }
                // ---- the slots' entries into the global accumulators ----
                if (slot + 1u == ZONAL_B || t + 1u == U.t1) {  // the slots 0 .. slot hold the instants t - slot .. t
                    __syncthreads();
                    for (uint32_t i = tid; i < (slot + 1u) * ZONAL_ZL; i += 256u) {
                        const uint32_t c = za[i].cnt;
                        if (c == 0) continue;
                        const int64_t ts = (int64_t)za[i].sum;
                        const int32_t tl = za[i].lo, th = za[i].hi;
                        za[i] = ZonalLds{0, 0u, INT32_MAX, INT32_MIN, 0u};
                        const uint64_t at = U.acc + (uint64_t)zlist[i % ZONAL_ZL] * U.a_st + (t - slot + i / ZONAL_ZL - U.t0);
                        zonal_add(acc, at, ts < 0 ? ~(uint64_t)0 : (uint64_t)0, (uint64_t)ts, space_scale(enc, C.fbits), c,
                                  EXT ? leaf_extreme(tl, INT32_MAX, enc, C.fbits, sg) : 0.0, EXT ? leaf_extreme(th, INT32_MIN, enc, C.fbits, sg) : 0.0, EXT, ADD);
                    }
                    slot = 0;
                } else {
                    slot += 1u;
                }
            }
        }
        __syncthreads();
        r0 += ZONAL_ZL;
        if (r0 >= n_distinct) {  // the unit's last round
            u += gridDim.x;
            r0 = 0;
        }
    }
}
#undef K2R_ZONAL_PUT
#undef K2R_ZONAL_LAB

int launch_bulk_zonal(const ChunkRef* d_refs, const uint8_t* d_enc, const ZonalUnit* d_units, uint32_t n, const uint16_t* d_labels,
                      uint32_t n_zones, uint64_t* d_acc, uint32_t live) {
    if (n == 0) return DCDF_OK;
    const dim3 grid = bulk_grid(n), block(256);
    constexpr uint32_t EXT = RA_MIN | RA_MAX, ADD = RA_SUM | RA_COUNT;
    const uint32_t l = ((live & EXT) ? EXT : 0u) | ((live & ADD) ? ADD : 0u);
#define K2R_ZONAL_CASE(L) \
    case L: hipLaunchKernelGGL((k_bulk_zonal<L>), grid, block, 0, 0, d_refs, d_enc, d_units, n, d_labels, n_zones, d_acc); break;
    switch (l) {
        K2R_ZONAL_CASE(EXT) K2R_ZONAL_CASE(ADD) K2R_ZONAL_CASE(EXT | ADD)
        default: return DCDF_ERR_BAD_ARG;
    }
#undef K2R_ZONAL_CASE
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- spell statistics (k2r_spell.h): the walk's cells into per-cell run states ----------------------------------------------
// plane_load4's rule in its 4-byte form: one 16-byte access when the four cells are inside and p is aligned, single elements
// otherwise.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void plane_load4u(const uint32_t* p, uint32_t (&v)[4], uint32_t c0, uint32_t left, uint32_t right) {
    if (c0 >= left && c0 + 4u <= right && ((uintptr_t)p & 15u) == 0) {
        const u32x4_t a = *(const __attribute__((address_space(1))) u32x4_t*)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c0 + (uint32_t)e >= left && c0 + (uint32_t)e < right) v[e] = ((const __attribute__((address_space(1))) uint32_t*)p)[e];
    }
}
__device__ __forceinline__ void plane_store4u(uint32_t* p, const uint32_t (&v)[4], uint32_t c0, uint32_t left, uint32_t right) {
    if (c0 >= left && c0 + 4u <= right && ((uintptr_t)p & 15u) == 0) {
        *(__attribute__((address_space(1))) u32x4_t*)p = u32x4_t{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (c0 + (uint32_t)e >= left && c0 + (uint32_t)e < right) ((__attribute__((address_space(1))) uint32_t*)p)[e] = v[e];
    }
}
// one state word of four cells of a row, between its plane and the threads' SpellStates
#define K2R_SPELL_LOAD(plane, field)                                                      \
    {                                                                                     \
        uint32_t w[4] = {st[a][0].field, st[a][1].field, st[a][2].field, st[a][3].field}; \
        plane_load4u((plane) + at, w, c0, left, right);                                   \
        _Pragma("unroll") for (uint32_t e = 0; e < 4u; e++) st[a][e].field = w[e];        \
    }
#define K2R_SPELL_STORE(plane, field)                                                           \
    {                                                                                           \
        const uint32_t w[4] = {st[a][0].field, st[a][1].field, st[a][2].field, st[a][3].field}; \
        plane_store4u((plane) + at, w, c0, left, right);                                        \
    }

// GROUPS: the state this instantiation carries -- SG_COUNT: count; SG_RUNS: cur, longest, lstart; SG_ENDS: first, last.  A thread
// owns the same 16 cells at every instant (its two tasks of 2 rows x 4 columns, bulk_cells8); their SpellStates stay in registers
// over the unit's instants and every instant is one spell_step per cell: integer compares with the leaf's range (spell_hit32),
// nothing is widened.  The state continues the planes': it is loaded before the first instant (spell_init when the unit starts
// its cube) and stored after the last.  Words of a group that is not carried are never loaded nor stored, so their updates are
// dead code.  Within a carried group a plane the caller did not ask for lives in scratch (spell_plane); FIRST without LAST (or the
// reverse) is carried in registers but only the requested plane is touched.  Cells outside the unit's rectangle are decoded as in
// k_bulk_decode; their rows are not accumulated and nothing of them is written.
template <uint32_t GROUPS>
__global__ void __launch_bounds__(256)
k_bulk_spell(const ChunkRef* __restrict__ chunks, const SpellUnit* __restrict__ units, uint32_t n_units, uint32_t* dst, uint32_t* scr, uint32_t ops) {
    typedef int32_t V;
    __shared__ V pyr[BP_SIZE];
    __shared__ uint32_t nst[BN_SIZE];
    __shared__ V nd[BN_SIZE];
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const SpellUnit U = units[u];
        const ChunkRef C = chunks[U.chunk];
        const gbytes gb = (gbytes)C.bytes;
        const uint32_t top = U.top, bottom = U.bottom, left = U.left, right = U.right;
        const int32_t lo = U.lo, hi = U.hi;
        const uint32_t flags = U.flags;
        uint32_t* const p_cnt = spell_plane(SP_COUNT, dst, scr, ops, U.o_off, U.s_off, U.psz);
        uint32_t* const p_lng = spell_plane(SP_LONGEST, dst, scr, ops, U.o_off, U.s_off, U.psz);
        uint32_t* const p_lst = spell_plane(SP_LSTART, dst, scr, ops, U.o_off, U.s_off, U.psz);
        uint32_t* const p_fst = spell_plane(SP_FIRST, dst, scr, ops, U.o_off, U.s_off, U.psz);
        uint32_t* const p_las = spell_plane(SP_LAST, dst, scr, ops, U.o_off, U.s_off, U.psz);
        uint32_t* const p_cur = spell_plane(SP_CUR, dst, scr, ops, U.o_off, U.s_off, U.psz);
        // states of row 2 k + i of the thread's cells
        SpellState st[4][4];
#pragma unroll
        for (uint32_t a = 0; a < 4u; a++) {
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) st[a][e] = spell_init();
            const uint32_t g = tid + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
            if (!U.init && r >= top && r < bottom && c0 + 4u > left && c0 < right) {
                const int64_t at = (int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left);
                if constexpr ((GROUPS & SG_COUNT) != 0) K2R_SPELL_LOAD(p_cnt, count)
                if constexpr ((GROUPS & SG_RUNS) != 0) {
                    K2R_SPELL_LOAD(p_cur, cur)
                    K2R_SPELL_LOAD(p_lng, longest)
                    if (ops & SP_LSTART) K2R_SPELL_LOAD(p_lst, lstart)
                }
                if constexpr ((GROUPS & SG_ENDS) != 0) {
                    if (ops & SP_FIRST) K2R_SPELL_LOAD(p_fst, first)
                    if (ops & SP_LAST) K2R_SPELL_LOAD(p_las, last)
                }
            }
        }
        uint32_t cur_snap = 0xffffffffu;
        for (uint32_t t = U.t0; t < U.t1; t++) {
            const BulkInstant I = bulk_instant(C, U, t, cur_snap, pyr, nst, nd, tid);
            const uint32_t ti = U.dt + (t - U.t0);  // counted from the cube's first instant
            // ---- nodes of side 2, two per task: their 2 x 4 cells, folded ----
#pragma unroll
            for (uint32_t k = 0; k < 2u; k++) {
                const uint32_t e = tid + 256u * k, rp = e >> 4, cg = e & 15u;
                const uint32_t r0 = (uint32_t)U.rr + 2u * rp, c0 = (uint32_t)U.rc + 4u * cg;  // chunk coordinates
                if (r0 + 2u <= top || r0 >= bottom || c0 + 4u <= left || c0 >= right) continue;
                V v[2][4];
                bulk_cells8(gb, I, pyr, nst, nd, rp, cg, v);
#pragma unroll
                for (uint32_t i = 0; i < 2u; i++) {
                    const uint32_t r = r0 + i, a = 2u * k + i;
                    if (r < top || r >= bottom) continue;
#pragma unroll
                    for (uint32_t c = 0; c < 4u; c++) spell_step(st[a][c], ti, spell_hit32(v[i][c], lo, hi, flags));
                }
            }
        }
        // ---- the unit's states into the planes ----
#pragma unroll
        for (uint32_t a = 0; a < 4u; a++) {
            const uint32_t g = tid + 256u * (a >> 1), r = (uint32_t)U.rr + 2u * (g >> 4) + (a & 1u), c0 = (uint32_t)U.rc + 4u * (g & 15u);
            if (r < top || r >= bottom || c0 + 4u <= left || c0 >= right) continue;
            const int64_t at = (int64_t)(r - top) * U.sr + ((int64_t)c0 - (int64_t)left);
            if constexpr ((GROUPS & SG_COUNT) != 0) K2R_SPELL_STORE(p_cnt, count)
            if constexpr ((GROUPS & SG_RUNS) != 0) {
                K2R_SPELL_STORE(p_cur, cur)
                K2R_SPELL_STORE(p_lng, longest)
                if (ops & SP_LSTART) K2R_SPELL_STORE(p_lst, lstart)
            }
            if constexpr ((GROUPS & SG_ENDS) != 0) {
                if (ops & SP_FIRST) K2R_SPELL_STORE(p_fst, first)
                if (ops & SP_LAST) K2R_SPELL_STORE(p_las, last)
            }
        }
        __syncthreads();
    }
}
#undef K2R_SPELL_LOAD
#undef K2R_SPELL_STORE

int launch_bulk_spell(const ChunkRef* d_refs, const SpellUnit* d_units, uint32_t n, uint32_t* d_dst, uint32_t* d_scr, uint32_t ops) {
    if (n == 0) return DCDF_OK;
    const dim3 grid = bulk_grid(n), block(256);
#define K2R_SPELL_CASE(G) \
    case G: hipLaunchKernelGGL((k_bulk_spell<G>), grid, block, 0, 0, d_refs, d_units, n, d_dst, d_scr, ops); break;
    switch (spell_groups(ops)) {
        K2R_SPELL_CASE(1) K2R_SPELL_CASE(2) K2R_SPELL_CASE(3) K2R_SPELL_CASE(4) K2R_SPELL_CASE(5) K2R_SPELL_CASE(6) K2R_SPELL_CASE(7)
        default: return DCDF_ERR_BAD_ARG;
    }
#undef K2R_SPELL_CASE
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

}  // namespace k2r
