// k2r_quantile.hip -- the selection kernel of dcdf_raster_quantile_time_batch (k2r_quantile.h; the call itself:
// k2r_raster_region.hip), and the same selection on the host.  Built with -ffp-contract=off (Makefile): the LINEAR method's
// subtraction, multiplication and addition stay three IEEE operations.
#include <hip/hip_runtime.h>

#include "../../include/dcdf_k2r.h"
#include "k2r_quantile.h"
#include "k2r_runtime.h"

using namespace k2r;

// A lane per cell of a column, a wave's 64 lanes on consecutive cells: every read of the slab is one contiguous segment per
// instant and wave.  The lane streams its cell's stored integers once per pass (quantile_cell) and widens them with the table
// entry of their segment; the pass loop ends when every cell of the wave is resolved.  Nothing but registers: R, the number of
// target ranks, is a template argument, and every loop over them unrolls.
template <uint32_t R>
__global__ void __launch_bounds__(256)
k_quantile_select(const QuantileCol* __restrict__ cols, uint32_t n, const QuantileSeg* __restrict__ segs, const int64_t* __restrict__ slab,
                  QuantileProbs probs, uint32_t n_probs, int32_t method, double* __restrict__ dst) {
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const QuantileCol P = cols[p];
        const uint64_t cells = (uint64_t)P.rows * P.cols;
        for (uint64_t e0 = (uint64_t)blockIdx.y * blockDim.x; e0 < cells; e0 += (uint64_t)gridDim.y * blockDim.x) {
            const uint64_t e = e0 + threadIdx.x;
            const bool on = e < cells;  // (a lane beyond the column repeats its last cell and stores nothing)
            const uint64_t ec = on ? e : cells - 1u;
            const int64_t* const src = slab + P.src + ec;
            double* const out = dst + P.o_off + ec / P.cols * P.sr + ec % P.cols;
            quantile_cell<R>(
                [&](auto&& f) {
                    for (uint32_t s = 0; s < P.nseg; s++) {
                        const QuantileSeg G = segs[P.seg0 + s];
                        const uint32_t t1 = s + 1u < P.nseg ? segs[P.seg0 + s + 1u].t0 : P.nt;
                        for (uint32_t t = G.t0; t < t1; t++) f(reduce_widen(G.enc, G.fbits, src[(uint64_t)t * cells]));
                    }
                },
                [](bool u) { return __ballot(u ? 1 : 0) != 0ull; },
                [&](uint32_t i, double v) {
                    if (on) out[(uint64_t)i * P.psz] = v;
                },
                probs.p, n_probs, method);
        }
    }
}

int k2r::launch_quantile_select(const QuantileCol* d_cols, uint32_t n, uint64_t max_cells, const QuantileSeg* d_segs, const int64_t* d_slab,
                                const QuantileProbs& probs, uint32_t n_probs, int32_t method, double* d_dst) {
    if (n == 0 || max_cells == 0) return DCDF_OK;
    const dim3 grid(std::min<uint32_t>(n, 1u << 20), (uint32_t)std::min<uint64_t>((max_cells + 255u) / 256u, 65535u)), block(256);
    // the target ranks a lane keeps in registers: 2 per probability
    if (n_probs <= 1u) hipLaunchKernelGGL(k_quantile_select<2>, grid, block, 0, 0, d_cols, n, d_segs, d_slab, probs, n_probs, method, d_dst);
    else if (n_probs <= 6u) hipLaunchKernelGGL(k_quantile_select<12>, grid, block, 0, 0, d_cols, n, d_segs, d_slab, probs, n_probs, method, d_dst);
    else hipLaunchKernelGGL(k_quantile_select<32>, grid, block, 0, 0, d_cols, n, d_segs, d_slab, probs, n_probs, method, d_dst);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

extern "C" int dcdf_quantile_select_host(const double* x, uint32_t instants, uint64_t cells, const double* probs, uint32_t n_probs, int32_t method,
                                         double* out, uint32_t* passes) {
    if (!x || !out || !quantile_args_ok(probs, n_probs, method)) return DCDF_ERR_BAD_ARG;
    for (uint64_t e = 0; e < cells; e++) {
        const uint32_t np = quantile_cell<2u * QUANTILE_MAX_PROBS>(
            [&](auto&& f) {
                for (uint32_t t = 0; t < instants; t++) f(x[(uint64_t)t * cells + e]);
            },
            [](bool u) { return u; }, [&](uint32_t i, double v) { out[(uint64_t)i * cells + e] = v; }, probs, n_probs, method);
        if (passes) passes[e] = np;
    }
    return DCDF_OK;
}
