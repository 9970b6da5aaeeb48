// k2r_rolling.hip -- the stream kernel of dcdf_raster_rolling_time_batch and dcdf_raster_rolling_time_groups_batch (k2r_rolling.h;
// the calls themselves: k2r_raster_region.hip).  Built with -ffp-contract=off (Makefile) as its siblings are; the arithmetic is
// integer but for the one rounding and the mean's one division.
#include <hip/hip_runtime.h>

#include "../../include/dcdf_k2r.h"
#include "k2r_rolling.h"
#include "k2r_runtime.h"

using namespace k2r;

// k_regress_stream's shape: a lane per cell of a column, a wave's 64 lanes on consecutive cells, so every read of the slab is
// one contiguous segment per instant and wave.  The lane walks its cell's windows group by group (rolling_cell): per instant of
// a run the entering value and the leaving one, w instants apart, both from the slab -- the tail is a second read of what the
// head read w instants earlier (DESIGN.md section 4o has what that costs).  It stores every plane's element itself: nothing is filled
// before or finished after.  The column, the windows' ends, the CSR, the instant table and the segment entries are indexed by
// values every lane of the workgroup shares.  Nothing but registers: no LDS, no atomics, no scratch.
__global__ void __launch_bounds__(256)
k_rolling_stream(const RollingCol* __restrict__ cols, uint32_t n, const QuantileSeg* __restrict__ segs, const uint32_t* __restrict__ ends,
                 const uint32_t* __restrict__ start, const uint32_t* __restrict__ seg_of, uint32_t n_groups, const int64_t* __restrict__ slab,
                 uint32_t ops, uint32_t window, uint32_t min_count, int32_t kind, double* __restrict__ dst) {
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const RollingCol P = cols[p];
        const uint64_t cells = (uint64_t)P.q.rows * P.q.cols;
        for (uint64_t e0 = (uint64_t)blockIdx.y * blockDim.x; e0 < cells; e0 += (uint64_t)gridDim.y * blockDim.x) {
            const uint64_t e = e0 + threadIdx.x;
            const bool on = e < cells;  // (a lane beyond the column repeats its last cell and stores nothing)
            const uint64_t ec = on ? e : cells - 1u;
            const int64_t* const src = slab + P.q.src + ec;
            double* const out = dst + P.q.o_off + ec / P.q.cols * P.q.sr + ec % P.q.cols;
            rolling_cell(
                ends + P.end0, start + P.start0, n_groups, seg_of + P.seg_of0, segs + P.q.seg0, ops, window, min_count, kind,
                [&](uint32_t t) { return src[(uint64_t)t * cells]; },
                [&](uint32_t i, double v) {
                    if (on) out[(uint64_t)i * P.q.psz] = v;
                });
        }
    }
}

int k2r::launch_rolling_stream(const RollingCol* d_cols, uint32_t n, uint64_t max_cells, const QuantileSeg* d_segs, const uint32_t* d_ends,
                               const uint32_t* d_start, const uint32_t* d_seg_of, uint32_t n_groups, const int64_t* d_slab, uint32_t ops,
                               uint32_t window, uint32_t min_count, int32_t kind, double* d_dst) {
    if (n == 0 || max_cells == 0) return DCDF_OK;
    const dim3 grid(std::min<uint32_t>(n, 1u << 20), (uint32_t)std::min<uint64_t>((max_cells + 255u) / 256u, 65535u)), block(256);
    hipLaunchKernelGGL(k_rolling_stream, grid, block, 0, 0, d_cols, n, d_segs, d_ends, d_start, d_seg_of, n_groups, d_slab, ops, window,
                       min_count, kind, d_dst);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}
