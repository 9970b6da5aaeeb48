// Stand-alone host program over plan_rolling_time (dcdf_amd/csrc/k2r_plan.h) and rolling_cell (k2r_rolling.h) (TEST INFRASTRUCTURE
// ONLY), built with -fsanitize=address,undefined by tests/test_rolling_host.py.  It runs the column stream of
// dcdf_raster_rolling_time_batch / _groups_batch on the CPU exactly as k_rolling_stream indexes it, before a card sees it: the
// geometries of tests/test_raster_plan_host.py (plain bulk, walk and checker tables, the tiled raster with an elided leaf), the
// slab cap at its default, at one that cuts rows and at one below a 64 x 64 part (every part alone in its band), batches of
// several cubes with one without instants and one without rows, five label sets (empty groups, 0xffff, labels >= n_groups, a
// first instant in no group, every instant its own group) and seven (window, min_count, kind) triples, one wider than any cube.
// For every band a host slab of EXACTLY the band's used elements is painted with each cell's own series; rolling_cell then runs
// for every column and every lane index the kernel forms, the lanes past the column's end included.  Checked: every slab read
// lies inside [0, used); every output element of every cube is written exactly once and nothing else is; the values have the
// bits of a loop written apart from the header -- its own 256-bit integers, every window summed again from its own values, the
// leaf looked up in the raster's table, its own rounding.  Prints "ok rolling <cases> <cells> <reads>".
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_plan.h"

using namespace k2r;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static uint64_t bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

// ---- the geometries (tests/sim/quantile_check.cpp's) -----------------------------------------------------------------------------
struct Geo {
    PlanRaster g;
    std::vector<PlanLeaf> leaves;
};
static Geo plain(int table) {  // 0: all bulk, 1: all walk, 2: checker
    Geo G;
    G.g = PlanRaster{20, 100, 200, 96, 9, 2, 3, nullptr};
    for (uint32_t leaf = 0; leaf < 18; leaf++) {
        const uint32_t seg = leaf / 6, ti = leaf / 3 % 2, tj = leaf % 3;
        G.leaves.push_back(PlanLeaf{0, 0, seg == 1 ? ENC_F32 : ENC_I32, seg, 0, (uint8_t)(table == 0 ? 1 : table == 1 ? 0 : (seg + ti + tj) % 2)});
    }
    return G;
}
static Geo tiled() {
    Geo G;
    G.g = PlanRaster{20, 40, 96, 32, 9, 2, 3, nullptr};
    const PlanLeaf seg[6] = {{0, 0, ENC_I32, 0, 0, 1}, {0, 32, ENC_I32, 0, 0, 1}, {0, 0, ENC_F32, 3, 1, 0},
                             {32, 0, ENC_I32, 0, 0, 1}, {32, 32, ENC_I32, 0, 0, 1}, {0, 0, ENC_I64, 0, 0, 0}};
    for (int s = 0; s < 3; s++)
        for (const PlanLeaf& L : seg) G.leaves.push_back(L);
    return G;
}

// ---- the painted raster: the stored integer of cell (R, C) at instant T -----------------------------------------------------------
static int64_t stored(uint32_t T, uint32_t R, uint32_t C) {
    if (R % 16 == 0 && C % 16 == 0) return 7;                 // a constant cell
    if (R % 16 == 1 && C % 16 == 1) return 0;                 // a float leaf's NaN on every instant
    if (R % 16 == 2 && C % 16 == 2) return T == 11 ? 5 : 0;   // one value (where the leaf is a float one)
    if (R % 16 == 3 && C % 16 == 3)                           // beyond 2^53 and near +-2^62: (double)n rounds, the sums need > 64 bits
        return T % 3 == 0 ? ((int64_t)1 << 53) + 1 + 2 * T : T % 3 == 1 ? ((int64_t)1 << 62) - 3 * T : -((int64_t)1 << 62) + 5 * T;
    if ((R + 2 * C + 3 * T) % 5 == 0) return 0;
    return (int64_t)((R * 131u + C * 71u + T * T * 17u + R * C % 13u) % 2001u) - 1000;
}
static double value_of(const PlanRaster& g, uint32_t T, uint32_t R, uint32_t C) {  // the leaf from the raster's own table
    const PlanLeaf& L = g.leaves[((uint64_t)(T / g.cs) * g.nti + R / g.tile) * g.ntj + C / g.tile];
    const int64_t n = stored(T, R, C);
    switch (L.enc) {
        case ENC_I32: return (double)(int32_t)n;
        case ENC_I64: return (double)n;
        case ENC_F32: return n == 0 ? std::nan("") : (double)((float)(n - 1) / (float)((int64_t)1 << (L.fbits + 1)));
        default: return n == 0 ? std::nan("") : (double)(n - 1) / (double)((int64_t)1 << (L.fbits + 1));
    }
}

// ---- the contract, written again: 256-bit two's complement integers at the 2^-63 scale ---------------------------------------------
struct Big {
    uint64_t w[4] = {0, 0, 0, 0};
    void add(const Big& b) {
        unsigned carry = 0;
        for (int i = 0; i < 4; i++) {
            const unsigned __int128 s = (unsigned __int128)w[i] + b.w[i] + carry;
            w[i] = (uint64_t)s;
            carry = (unsigned)(s >> 64);
        }
    }
    Big negated() const {
        Big r, one;
        for (int i = 0; i < 4; i++) r.w[i] = ~w[i];
        one.w[0] = 1;
        r.add(one);
        return r;
    }
    bool negative() const { return (w[3] >> 63) != 0; }
    bool less(const Big& b) const {  // signed
        if (negative() != b.negative()) return negative();
        for (int i = 3; i >= 0; i--)
            if (w[i] != b.w[i]) return w[i] < b.w[i];
        return false;
    }
    bool bit(int i) const { return i >= 0 && ((w[i >> 6] >> (i & 63)) & 1u) != 0; }
    // x * 2^63 of a double that is a multiple of 2^-63
    static Big of(double x) {
        int e;
        const double f = std::frexp(x, &e);                  // x = f * 2^e, 0.5 <= |f| < 1
        const int64_t m = (int64_t)std::ldexp(f, 53);        // exact: 53 bits
        const int sh = e - 53 + 63;
        CHECK(sh >= 0 && sh < 128);
        Big r;
        const uint64_t a = (uint64_t)(m < 0 ? -m : m);
        r.w[sh >> 6] = a << (sh & 63);
        if (sh & 63) r.w[(sh >> 6) + 1] = a >> (64 - (sh & 63));
        return m < 0 ? r.negated() : r;
    }
    // this / 2^63 as the nearest double, ties to even
    double rounded() const {
        const bool neg = negative();
        const Big m = neg ? negated() : *this;
        int p = 255;
        while (p >= 0 && !m.bit(p)) p--;
        if (p < 0) return 0.0;
        uint64_t q = 0;
        const int low = p > 52 ? p - 52 : 0;
        for (int i = p; i >= low; i--) q = (q << 1) | (m.bit(i) ? 1u : 0u);
        if (low > 0 && m.bit(low - 1)) {
            bool rest = false;
            for (int i = low - 2; i >= 0; i--) rest = rest || m.bit(i);
            if (rest || (q & 1u)) q++;
        }
        const double r = std::ldexp((double)q, low - 63);
        return neg ? -r : r;
    }
};

// ---- one case ----------------------------------------------------------------------------------------------------------------------
struct Totals {
    uint64_t cases = 0, cells = 0, reads = 0, bands = 0, alone = 0, lanes_past = 0, none = 0, one = 0, differ = 0, wide = 0;
};
// label set: 0 the plain call; 1: five groups, group 4 empty, 0xffff first, labels >= n_groups among them; 2: pairs (t / 2) with
// a 0xffff inside; 3: every instant its own group; 4: one group of zeros
static uint32_t label_of(int set, uint32_t t) {
    switch (set) {
        case 1: return t == 0 ? 0xffffu : t % 7 == 3 ? 9u : t % 6 == 5 ? 5u : (t * 3u) % 4u;
        case 2: return t == 5 ? 0xffffu : t / 2;
        case 3: return t;
        default: return 0;
    }
}
struct Params {
    uint32_t window, min_count;
    int32_t kind;
};
static void run_case(Geo& G, const std::vector<dcdf_cube>& cubes, bool node_wise, uint64_t cap_bytes, int set, Params pr, uint32_t ops, Totals& tot) {
    G.g.leaves = G.leaves.data();
    const PlanRaster& g = G.g;
    const size_t nq = cubes.size();
    const uint32_t n_groups = set == 0 || set == 4 ? 1u : set == 1 ? 5u : set == 2 ? 10u : g.T;
    const uint32_t w = pr.window;
    uint32_t n_planes = 0;
    for (uint32_t k = 0; k < 5; k++) n_planes += ops >> k & 1u;
    n_planes *= n_groups;
    // the arrays of the call: outputs with odd gaps, labels per cube with gaps of their own
    std::vector<dcdf_cube> nc(nq);
    std::vector<uint64_t> base(nq), plane(nq), loff(nq);
    std::vector<uint16_t> labels;
    uint64_t at = 0;
    for (size_t q = 0; q < nq; q++) {
        nc[q] = norm_cube(cubes[q]);
        plane[q] = cube_cells(nc[q]) ? (uint64_t)(nc[q].bottom - nc[q].top) * (nc[q].right - nc[q].left) : 0;
        base[q] = at + 3 + q % 2;
        at = base[q] + n_planes * plane[q];
        labels.push_back(0);  // (a gap)
        loff[q] = labels.size();
        for (uint32_t t = 0; t < nc[q].end - nc[q].start; t++) labels.push_back((uint16_t)label_of(set, t));
    }
    const uint64_t total = at + 5;
    RollingPlan P;
    CHECK(plan_rolling_time(g, cubes.data(), nq, base.data(), cap_bytes, node_wise, 64, ops, w, pr.min_count, pr.kind, set ? labels.data() : nullptr,
                            set ? loff.data() : nullptr, n_groups, P) == DCDF_OK);
    CHECK(P.cols.size() == P.q.cols.size() && P.q.col_cube.size() == P.cols.size());
    // the tables of every cube: the segment of every instant, the windows' ends sorted by (label, instant), the CSR over them
    std::vector<uint32_t> cube_end0(nq, 0), cube_start0(nq, 0), cube_seg0(nq, 0);
    {
        uint32_t e0 = 0, s0 = 0, g0 = 0;
        for (size_t q = 0; q < nq; q++) {
            if (!plane[q]) continue;
            cube_end0[q] = e0, cube_start0[q] = s0, cube_seg0[q] = g0;
            const uint32_t nt = nc[q].end - nc[q].start;
            CHECK(g0 + nt <= P.seg_of.size());
            for (uint32_t t = 0; t < nt; t++) CHECK(P.seg_of[g0 + t] == (nc[q].start + t) / g.cs - nc[q].start / g.cs);
            CHECK(s0 + n_groups + 1 <= P.start.size() && P.start[s0] == 0);
            uint32_t k = 0;
            for (uint32_t gr = 0; gr < n_groups; gr++) {
                CHECK(P.start[s0 + gr] == k);
                for (uint32_t t = w - 1; t < nt; t++) {
                    if ((set ? labels[loff[q] + t] : 0u) != gr) continue;
                    CHECK(e0 + k < P.ends.size() && P.ends[e0 + k] == t);
                    k++;
                }
            }
            CHECK(P.start[s0 + n_groups] == k);
            e0 += k, s0 += n_groups + 1, g0 += nt;
        }
        CHECK(e0 == P.ends.size() && s0 == P.start.size() && g0 == P.seg_of.size());
    }
    std::vector<uint8_t> written(total, 0);
    std::vector<double> out(total, -12345.0);
    for (const QuantileBand& b : P.q.bands) {
        uint64_t used = 0;
        for (size_t i = b.col0; i < b.col1; i++) used += (uint64_t)P.cols[i].q.nt * P.cols[i].q.rows * P.cols[i].q.cols;
        CHECK(used <= P.q.slab_max && used > 0);
        tot.bands++;
        tot.alone += b.col1 - b.col0 == 1;
        std::vector<int64_t> slab(used);  // exactly: one element further is the sanitizer's
        // paint: what the band's decode leaves there, dense [nt][rows][cols] per column from its src
        for (size_t i = b.col0; i < b.col1; i++) {
            const QuantileCol& c = P.cols[i].q;
            const size_t q = P.q.col_cube[i];
            CHECK(q < nq && plane[q] && P.cols[i].end0 == cube_end0[q] && P.cols[i].start0 == cube_start0[q] && P.cols[i].seg_of0 == cube_seg0[q]);
            CHECK(c.o_off >= base[q] && c.o_off < base[q] + plane[q] && c.psz == plane[q] && c.nt == nc[q].end - nc[q].start);
            const uint64_t p = c.o_off - base[q];
            const uint32_t R0 = nc[q].top + (uint32_t)(p / c.sr), C0 = nc[q].left + (uint32_t)(p % c.sr);
            for (uint32_t t = 0; t < c.nt; t++)
                for (uint32_t r = 0; r < c.rows; r++)
                    for (uint32_t cc = 0; cc < c.cols; cc++) {
                        const uint64_t at_slab = c.src + ((uint64_t)t * c.rows + r) * c.cols + cc;
                        CHECK(at_slab < used);
                        slab[at_slab] = stored(nc[q].start + t, R0 + r, C0 + cc);
                    }
        }
        // the launch: blockIdx.x strides the band's columns, blockIdx.y blocks of 256 cells, as launch_rolling_stream sizes them
        const uint32_t gy = (uint32_t)std::min<uint64_t>((b.max_cells + 255u) / 256u, 65535u);
        for (size_t i = b.col0; i < b.col1; i++) {
            const RollingCol& Pc = P.cols[i];
            const size_t q = P.q.col_cube[i];
            const uint64_t cells = (uint64_t)Pc.q.rows * Pc.q.cols;
            CHECK(cells <= b.max_cells && Pc.q.seg0 + Pc.q.nseg <= P.q.segs.size());
            const uint64_t p = Pc.q.o_off - base[q];
            const uint32_t R0 = nc[q].top + (uint32_t)(p / Pc.q.sr), C0 = nc[q].left + (uint32_t)(p % Pc.q.sr);
            for (uint32_t by = 0; by < gy; by++)
                for (uint64_t e0 = (uint64_t)by * 256u; e0 < cells; e0 += (uint64_t)gy * 256u)
                    for (uint32_t tid = 0; tid < 256u; tid++) {
                        const uint64_t e = e0 + tid;
                        const bool on = e < cells;
                        const uint64_t ec = on ? e : cells - 1u;
                        tot.lanes_past += !on;
                        const uint64_t src = Pc.q.src + ec;
                        const uint64_t o = Pc.q.o_off + ec / Pc.q.cols * Pc.q.sr + ec % Pc.q.cols;
                        const uint32_t R = R0 + (uint32_t)(ec / Pc.q.cols), C = C0 + (uint32_t)(ec % Pc.q.cols);
                        uint32_t puts = 0;
                        rolling_cell(
                            P.ends.data() + Pc.end0, P.start.data() + Pc.start0, n_groups, P.seg_of.data() + Pc.seg_of0, P.q.segs.data() + Pc.q.seg0,
                            ops, w, pr.min_count, pr.kind,
                            [&](uint32_t t) {
                                const uint64_t idx = src + (uint64_t)t * cells;
                                CHECK(t < Pc.q.nt && idx < used);
                                tot.reads++;
                                return slab[idx];
                            },
                            [&](uint32_t pl, double v) {
                                puts++;
                                if (!on) return;
                                CHECK(pl < n_planes);
                                const uint64_t idx = o + (uint64_t)pl * Pc.q.psz;
                                CHECK(idx >= base[q] && idx < base[q] + n_planes * plane[q] && written[idx] == 0);
                                written[idx] = 1;
                                out[idx] = v;
                            });
                        CHECK(puts == n_planes);
                        if (!on) continue;
                        tot.cells++;
                        // the reference of this cell, group by group: every window summed again
                        for (uint32_t gr = 0; gr < n_groups; gr++) {
                            Big mx, mn;
                            uint32_t amx = 0, amn = 0, valid = 0;
                            for (uint32_t t = w - 1; t < Pc.q.nt; t++) {
                                if ((set ? labels[loff[q] + t] : 0u) != gr) continue;
                                Big S;
                                uint32_t cnt = 0;
                                for (uint32_t u = t + 1 - w; u <= t; u++) {
                                    const double x = value_of(g, nc[q].start + u, R, C);
                                    if (x != x) continue;
                                    S.add(Big::of(x));
                                    cnt++;
                                }
                                if (cnt < pr.min_count) continue;
                                if (valid == 0 || mx.less(S)) mx = S, amx = t;
                                if (valid == 0 || S.less(mn)) mn = S, amn = t;
                                valid++;
                            }
                            const double nan = std::nan("");
                            double hi = mx.rounded(), lo = mn.rounded();
                            if (pr.kind == 1) {
                                volatile double a = hi / (double)w, c2 = lo / (double)w;
                                hi = a, lo = c2;
                            }
                            const double want[5] = {valid ? hi : nan, valid ? (double)amx : nan, valid ? lo : nan, valid ? (double)amn : nan, (double)valid};
                            tot.none += valid == 0;
                            tot.one += valid == 1;
                            tot.differ += valid && amx != amn;
                            tot.wide += valid && (mx.w[1] != 0 && mx.w[1] != ~(uint64_t)0);
                            uint32_t pl = gr;
                            for (uint32_t k = 0; k < 5; k++)
                                if (ops >> k & 1u) {
                                    const double got = out[o + (uint64_t)pl * Pc.q.psz];
                                    if (bits(got) != bits(want[k])) {
                                        std::printf("FAILED value: cube %zu cell (%u, %u) group %u statistic %u window %u min_count %u kind %d: %.17g, want %.17g\n",
                                                    q, R, C, gr, k, w, pr.min_count, pr.kind, got, want[k]);
                                        std::exit(1);
                                    }
                                    pl += n_groups;
                                }
                        }
                    }
        }
    }
    // every element of every cube's planes exactly once, nothing else
    uint64_t n_written = 0, n_want = 0;
    for (uint8_t x : written) n_written += x;
    for (size_t q = 0; q < nq; q++) {
        n_want += n_planes * plane[q];
        for (uint64_t i = 0; i < n_planes * plane[q]; i++) CHECK(written[base[q] + i] == 1);
    }
    CHECK(n_written == n_want);
    tot.cases++;
}

int main() {
    Totals tot;
    const uint32_t ops_of[5] = {31u, 2u, 21u, 31u, 10u};
    // (window, min_count, kind): 21 is wider than any cube here -- no window anywhere
    const Params params[7] = {{1, 1, 0}, {2, 1, 0}, {5, 5, 1}, {5, 2, 0}, {8, 8, 0}, {9, 3, 0}, {21, 1, 0}};
    uint32_t turn = 0;  // 7 triples against 5 label sets: every pair of the two meets
    for (int geo = 0; geo < 4; geo++) {
        Geo G = geo < 3 ? plain(geo) : tiled();
        const uint32_t T = G.g.T, R = G.g.R, C = G.g.C;
        const dcdf_cube inner = geo < 3 ? dcdf_cube{1, 19, 33, 99, 63, 193} : dcdf_cube{1, 19, 5, 39, 20, 90};
        std::vector<dcdf_cube> cubes = {{0, T, 0, R, 0, C}, {T - 2, T - 1, R / 2, R / 2 + 1, C - 1, C}, {4, 4, 0, R, 0, C}, inner, {0, T, 7, 7, 1, C},
                                        {inner.end, inner.start, inner.bottom, inner.top, inner.right, inner.left}};
        std::vector<dcdf_cube> rev(cubes.rbegin(), cubes.rend());
        for (int node_wise = 0; node_wise < 2; node_wise++)
            // a cap below one 64 x 64 part (every part alone in its band), one that cuts rows only, the library's default
            for (uint64_t cap : {(uint64_t)1000, (uint64_t)20 * 64 * 96 * 8, (uint64_t)256 << 20})
                for (int set = 0; set < 5; set++) {
                    run_case(G, cubes, node_wise != 0, cap, set, params[turn++ % 7], ops_of[set], tot);
                    if (cap == 1000) run_case(G, rev, node_wise != 0, cap, set, params[turn++ % 7], ops_of[(set + 1) % 5], tot);
                }
    }
    CHECK(tot.alone > 100 && tot.lanes_past > 0);
    CHECK(tot.none > 0 && tot.one > 0 && tot.differ > 0 && tot.wide > 0);
    // the call's own arguments: refused before any plan is made
    {
        Geo G = plain(0);
        G.g.leaves = G.leaves.data();
        const dcdf_cube cube[1] = {{0, 3, 0, 4, 0, 4}};
        const uint64_t base[1] = {0};
        const uint32_t bad[][4] = {{0, 2, 1, 0},  {32, 2, 1, 0}, {1, 0, 1, 0}, {1, 65536, 1, 0}, {1, 2, 0, 0},
                                   {1, 2, 3, 0},  {1, 2, 1, 2},  {1, 2, 1, 1}, {1, 1, 0, 1}};
        for (const auto& b : bad) {
            RollingPlan P;
            CHECK(plan_rolling_time(G.g, cube, 1, base, 1 << 20, false, 64, b[0], b[1], b[2], (int32_t)b[3], nullptr, nullptr, 1, P) == DCDF_ERR_BAD_ARG);
            CHECK(P.ends.empty() && P.start.empty() && P.seg_of.empty() && P.cols.empty());
        }
        RollingPlan P;
        CHECK(plan_rolling_time(G.g, cube, 1, base, 1 << 20, false, 64, 1, 2, 1, -1, nullptr, nullptr, 1, P) == DCDF_ERR_BAD_ARG);
        CHECK(plan_rolling_time(G.g, cube, 1, base, 1 << 20, false, 64, 31, 65535, 65535, 1, nullptr, nullptr, 1, P) == DCDF_OK && P.ends.empty());
    }
    std::printf("ok rolling %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot.cases, tot.cells, tot.reads);
    return 0;
}
