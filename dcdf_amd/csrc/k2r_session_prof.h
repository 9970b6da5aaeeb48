// k2r_session_prof.h -- what K2R_PROFILE_PRINT prints after a run (k2r_capi_encode.hip only): the phase cycles the kernels left in
// the tiles' results, summed; per wave too in a -DK2R_PROFILE build.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "k2r_common.h"

namespace k2r {

inline void print_profile(const TileResult* results, size_t n) {
    uint64_t acc[NPROF] = {0};
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < NPROF; k++) acc[k] += results[i].prof[k];
    uint64_t tot = 0;
    for (int k = 0; k < NPROF; k++) tot += acc[k];
    static const char* names[NPROF] = {"p1 load+analysis", "p2 top", "p3 own/top nodes", "reduce4", "clear+hdr",
                                       "emit C snapshot", "emit C/Q log", "T/eqB bitmaps", "Lmax dac | V0,M0 bitmaps", "Lmin dac | zero bitmaps",
                                       "emit pass A", "emit pass B/I", "sizes+heuristic", "winner scan", "byte-1 pass A", "fast: phase 1",
                                       "fast: wait p1", "fast: top+plan", "fast: copy-out", "fast: bitmaps"};
    for (int k = 0; k < NPROF; k++)
        std::fprintf(stderr, "k2r-prof %-18s %14llu cyc %5.1f%%\n", names[k], (unsigned long long)acc[k],
                     tot ? 100.0 * (double)acc[k] / (double)tot : 0.0);
#ifdef K2R_PROFILE
    // Per WAVE (k2r_exec.h): cycles of a wave's own work and cycles it was parked at barriers, per phase, summed over all
    // tiles.  "max" is the busiest wave's work -- what the phase costs the workgroup --, "mean" the average wave's; the
    // difference is barrier wait caused by imbalance, and "wait" is what the average wave actually spent parked.
    {
        static uint64_t w[16][NPROF][2];
        std::memset(w, 0, sizeof(w));
        for (size_t i = 0; i < n; i++)
            for (int v = 0; v < 16; v++)
                for (int k = 0; k < NPROF; k++) {
                    w[v][k][0] += results[i].pw[v][k][0];
                    w[v][k][1] += results[i].pw[v][k][1];
                }
        int nw = 0;
        for (int v = 0; v < 16; v++) {
            uint64_t t = 0;
            for (int k = 0; k < NPROF; k++) t += w[v][k][0] + w[v][k][1];
            if (t) nw = v + 1;
        }
        uint64_t insts = 0;
        for (size_t i = 0; i < n; i++) insts += results[i].snapshots + results[i].logs;
        double all = 0;
        for (int k = 0; k < NPROF; k++)
            for (int v = 0; v < nw; v++) all += (double)(w[v][k][0] + w[v][k][1]);
        all /= nw ? nw : 1;
        std::fprintf(stderr, "k2r-pw %d waves, %llu chunk-instants, %.0f cycles per chunk-instant and wave (work + wait)\n", nw,
                     (unsigned long long)insts, insts ? all / (double)insts : 0.0);
        std::fprintf(stderr, "k2r-pw %-24s %9s %9s %9s %9s %7s   (cycles per chunk-instant)\n", "phase", "work-mean", "work-max", "work-w0",
                     "wait-mean", "share");
        for (int k = 0; k < NPROF; k++) {
            double mean = 0, mx = 0, wait = 0;
            for (int v = 0; v < nw; v++) {
                mean += (double)w[v][k][0];
                wait += (double)w[v][k][1];
                mx = std::max(mx, (double)w[v][k][0]);
            }
            if (mean + wait == 0) continue;
            mean /= nw;
            wait /= nw;
            const double d = insts ? (double)insts : 1.0;
            std::fprintf(stderr, "k2r-pw %-24s %9.0f %9.0f %9.0f %9.0f %6.1f%%\n", names[k], mean / d, mx / d, (double)w[0][k][0] / d, wait / d,
                         all ? 100.0 * (mean + wait) / all : 0.0);
        }
        // Every wave of every phase: which wave is the busy one decides where work can be moved to.
        const double d = insts ? (double)insts : 1.0;
        for (int c = 0; c < 2; c++) {
            std::fprintf(stderr, "k2r-pw-%s %-24s", c ? "wait" : "work", "phase \\ wave");
            for (int v = 0; v < nw; v++) std::fprintf(stderr, " %6d", v);
            std::fprintf(stderr, "\n");
            for (int k = 0; k < NPROF; k++) {
                uint64_t any = 0;
                for (int v = 0; v < nw; v++) any += w[v][k][0] + w[v][k][1];
                if (!any) continue;
                std::fprintf(stderr, "k2r-pw-%s %-24s", c ? "wait" : "work", names[k]);
                for (int v = 0; v < nw; v++) std::fprintf(stderr, " %6.0f", (double)w[v][k][c] / d);
                std::fprintf(stderr, "\n");
            }
        }
        // Phases with no barrier between them form a group: a wave runs through the group at its own pace, so the group costs
        // the workgroup the largest per-wave SUM of work, not the sum of the per-phase maxima.  Every other phase is a group of
        // its own.  (The third group wraps around: the tail of one instant runs into phase 1 of the next.)
        static const struct { const char* name; int n; int k[3]; } groups[] = {
            {"A + I + Q records", 3, {10, 11, 6}}, {"replay + zero bm + p1", 3, {14, 9, 0}}, {"p3 + scan", 2, {2, 3}},
            {"p2 top", 1, {1}}, {"sizes+heuristic", 1, {12}}, {"clear+hdr", 1, {4}}, {"V0,M0 bitmaps", 1, {8}},
            {"emit C snapshot", 1, {5}}, {"T/eqB bitmaps", 1, {7}}};
        std::fprintf(stderr, "k2r-pw-group %-24s", "group \\ wave");
        for (int v = 0; v < nw; v++) std::fprintf(stderr, " %6d", v);
        std::fprintf(stderr, " %7s %7s\n", "max", "mean");
        double crit = 0, avg = 0;
        for (const auto& g : groups) {
            double mx = 0, mean = 0;
            std::fprintf(stderr, "k2r-pw-group %-24s", g.name);
            for (int v = 0; v < nw; v++) {
                double s = 0;
                for (int i = 0; i < g.n; i++) s += (double)w[v][g.k[i]][0];
                std::fprintf(stderr, " %6.0f", s / d);
                mx = std::max(mx, s);
                mean += s;
            }
            mean /= nw ? nw : 1;
            std::fprintf(stderr, " %7.0f %7.0f\n", mx / d, mean / d);
            crit += mx;
            avg += mean;
        }
        std::fprintf(stderr, "k2r-pw-group sum of the group maxima %.0f, of the group means %.0f, imbalance %.0f (cycles per chunk-instant)\n",
                     crit / d, avg / d, (crit - avg) / d);
    }
#endif
    // per-tile totals: how uneven are the chunks?  (cycles per instant, logs that did not come from the stash)
    std::vector<double> per;
    uint64_t logs = 0, stash = 0;
    for (size_t i = 0; i < n; i++) {
        uint64_t t = 0;
        for (int k = 0; k < NPROF; k++) t += results[i].prof[k];
        const uint32_t ni = results[i].snapshots + results[i].logs;
        if (ni) per.push_back((double)t / ni);
        logs += results[i].logs;
        stash += results[i].stash_logs;
    }
    std::sort(per.begin(), per.end());
    if (!per.empty()) {
        double sum = 0;
        for (double x : per) sum += x;
        std::fprintf(stderr, "k2r-prof cycles/instant per tile: min %.0f p50 %.0f mean %.0f p90 %.0f p99 %.0f max %.0f | logs %llu from stash %llu\n",
                     per.front(), per[per.size() / 2], sum / per.size(), per[per.size() * 9 / 10], per[per.size() * 99 / 100],
                     per.back(), (unsigned long long)logs, (unsigned long long)stash);
    }
}

}  // namespace k2r
