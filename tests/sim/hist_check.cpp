// Stand-alone host program over the K2R_HD helpers of dcdf_amd/csrc/k2r_hist.h (TEST INFRASTRUCTURE ONLY): the translation of
// histogram edges into stored integers and the fold's binning, run on a CPU -- built with -fsanitize=address,undefined by
// tests/test_histogram_host.py.  Reads commands from the file named on the command line, prints one line per command:
//   L enc fbits bins (edge bits, hex) * (bins + 1)  k  n * k
//       a leaf and k stored integers: prints per integer "a b c" --
//       a = its bin by the inclusive intervals (hist_intervals; -1 none, -3 more than one),
//       b = its bin by the bulk kernel's int32 threshold table and branch-free search (hist_thresholds32, hist_search32;
//           -2 when |n| > 2^30, which a narrow32 chunk never stores, or n is the NaN code),
//       c = its bin by the fold's rule on the decoded value (hist_bin of from_fixed / (double)n; NaN code: -1).
//   then "ok" or "bad" for hist_edges_ok && hist_leaf_ok (a bad command prints "bad" alone)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_hist.h"

using namespace k2r;

static double widen(int32_t enc, uint32_t fbits, int64_t n) {  // reduce_widen (k2r_reduce.h)
    switch (enc) {
        case ENC_I32: return (double)(int32_t)n;
        case ENC_I64: return (double)n;
        case ENC_F32: return n == 0 ? __builtin_nan("") : (double)from_fixed_f32(n, fbits);
        default: return n == 0 ? __builtin_nan("") : from_fixed_f64(n, fbits);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char cmd;
    while (std::fscanf(f, " %c", &cmd) == 1) {
        if (cmd != 'L') return 3;
        int32_t enc;
        uint32_t fbits, bins;
        if (std::fscanf(f, "%" SCNd32 " %" SCNu32 " %" SCNu32, &enc, &fbits, &bins) != 3 || bins > 100000u) return 3;
        std::vector<double> edges(bins + 1);
        for (uint32_t j = 0; j <= bins; j++) {
            uint64_t b;
            if (std::fscanf(f, "%" SCNx64, &b) != 1) return 3;
            std::memcpy(&edges[j], &b, sizeof b);
        }
        size_t k;
        if (std::fscanf(f, "%zu", &k) != 1) return 3;
        std::vector<int64_t> ns(k);
        for (size_t i = 0; i < k; i++)
            if (std::fscanf(f, "%" SCNd64, &ns[i]) != 1) return 3;
        if (!hist_edges_ok(edges.data(), bins) || !hist_leaf_ok(enc, fbits)) {
            std::printf("bad\n");
            continue;
        }
        std::vector<int64_t> lo(bins), hi(bins);
        hist_intervals(enc, fbits, edges.data(), bins, lo.data(), hi.data());
        const uint32_t steps = hist_steps(bins);
        std::vector<int32_t> thr((size_t)1 << steps);
        hist_thresholds32(enc, fbits, edges.data(), bins, thr.data(), (uint32_t)thr.size());
        const bool rev = hist_reversed(enc, fbits);
        for (int64_t n : ns) {
            int a = -1;
            for (uint32_t b = 0; b < bins; b++)
                if (lo[b] <= n && n <= hi[b]) a = a == -1 ? (int)b : -3;
            int b32 = -2;
            if (n >= -((int64_t)1 << 30) && n <= ((int64_t)1 << 30) && !(hist_float(enc) && n == 0)) {
                const int32_t p = hist_search32(thr.data(), steps, (int32_t)n);
                b32 = p < 0 || p >= (int32_t)bins ? -1 : rev ? (int)bins - 1 - p : p;
            }
            std::printf("%d %d %d ", a, b32, (int)hist_bin(edges.data(), bins, widen(enc, fbits, n)));
        }
        std::printf("ok\n");
    }
    std::fclose(f);
    return 0;
}
