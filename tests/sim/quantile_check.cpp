// Stand-alone host program over dcdf_amd/csrc/k2r_quantile.h and plan_quantile_time of k2r_plan.h (TEST INFRASTRUCTURE ONLY), built
// with -fsanitize=address,undefined by tests/test_quantile_host.py.  Five checks, each printing "ok <name> <count>":
//   (a) keys    quantile_key is strictly monotone over a table of doubles (+-0, denormals, +-2^62, neighbours by nextafter, +-inf)
//               and quantile_unkey(quantile_key(x)) is x bit for bit;
//   (b) small   the selection loop of the kernel (quantile_cell, this header compiled for the host) agrees with std::sort and the
//               rank rule written out again here for EVERY series of length <= 7 over four values and NaN -- ties, all-equal and
//               all-NaN series among them --, every method, p in {0, 0.1, 0.5, 0.9, 1}, alone and all five in one call;
//   (c) random  the same for 10 000 random series of length 1 .. 400 whose keys share a long prefix and differ in low bits, with
//               1 .. 16 probabilities a call;
//   (d) plan    plan_quantile_time on the geometries of tests/test_raster_plan_host.py: every cell of every cube lies in exactly
//               one column, every band is under the cap unless it is one column, the column tables cover the cube's instants
//               without gap with the leaves' own encodings, and everything the band's decode writes lies inside its slab;
//   (e) ranks   quantile_rank against integer arithmetic where (n - 1) p is exact.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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
static bool same(double a, double b) { return (a != a && b != b) || bits(a) == bits(b); }

// ---- (a) ---------------------------------------------------------------------------------------------------------------------
static uint64_t check_keys() {
    const double inf = std::numeric_limits<double>::infinity(), dmin = std::numeric_limits<double>::denorm_min();
    std::vector<double> seed = {0.0, dmin, 3 * dmin, std::numeric_limits<double>::min(), 1.0, 1.5, 4611686018427387904.0 /* 2^62 */, 1e300,
                                std::numeric_limits<double>::max()};
    std::vector<double> t;
    for (double s : seed)
        for (double x : {std::nextafter(s, -inf), s, std::nextafter(s, inf)})
            if (x >= 0.0 && !(x == 0.0 && std::signbit(x))) t.push_back(x);
    t.push_back(inf);
    std::sort(t.begin(), t.end());
    t.erase(std::unique(t.begin(), t.end()), t.end());
    std::vector<double> all;  // ascending: -inf .. -0.0, +0.0 .. +inf
    for (size_t i = t.size(); i-- > 0;) all.push_back(-t[i]);
    for (double x : t) all.push_back(x);
    CHECK(std::signbit(all[t.size() - 1]) && all[t.size() - 1] == 0.0 && !std::signbit(all[t.size()]) && all[t.size()] == 0.0);
    for (size_t i = 0; i < all.size(); i++) {
        CHECK(bits(quantile_unkey(quantile_key(all[i]))) == bits(all[i]));
        if (i) CHECK(quantile_key(all[i - 1]) < quantile_key(all[i]));  // strictly: -0.0 below +0.0 too
    }
    return all.size();
}

// ---- the reference: sort, then the rank rule written apart from quantile_rank / quantile_finish ---------------------------------
static bool below(double a, double b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }
static double reference(std::vector<double> v, double p, int method) {  // v: the non-NaN values
    if (v.empty()) return std::nan("");
    std::sort(v.begin(), v.end(), below);
    const size_t n = v.size();
    const double h = (double)(n - 1) * p, fl = std::floor(h), g = h - fl;
    const size_t j = (size_t)fl, j1 = std::min(j + 1, n - 1);
    if (method == 0) return v[j];
    if (method == 1) return g == 0.0 ? v[j] : v[j1];
    if (method == 2) return g < 0.5 ? v[j] : g > 0.5 ? v[j1] : (j % 2 == 0 ? v[j] : v[j1]);
    if (g == 0.0) return v[j];
    volatile double d = v[j1] - v[j];
    volatile double m = d * g;
    return v[j] + m;
}
template <uint32_t R>
static uint32_t select(const std::vector<double>& x, const double* probs, uint32_t n_probs, int method, double* out) {
    return quantile_cell<R>(
        [&](auto&& f) {
            for (double e : x) f(e);
        },
        [](bool u) { return u; }, [&](uint32_t i, double v) { out[i] = v; }, probs, n_probs, method);
}
static void check_series(const std::vector<double>& x, const double* probs, uint32_t n_probs) {
    std::vector<double> v;
    for (double e : x)
        if (e == e) v.push_back(e);
    for (int method = 0; method < 4; method++) {
        double got[QUANTILE_MAX_PROBS], big[QUANTILE_MAX_PROBS], one[1];
        const uint32_t np = n_probs <= 1 ? select<2>(x, probs, n_probs, method, got)
                            : n_probs <= 6 ? select<12>(x, probs, n_probs, method, got) : select<32>(x, probs, n_probs, method, got);
        CHECK(np <= 2u * n_probs * 22u);  // (64 bits, 3 a pass)
        if (n_probs <= 6) CHECK(select<32>(x, probs, n_probs, method, big) == np);  // the kernel's largest form: the same passes
        for (uint32_t i = 0; i < n_probs; i++) {
            const double want = reference(v, probs[i], method);
            CHECK(same(got[i], want));
            if (n_probs <= 6) CHECK(same(big[i], want));
            if (n_probs > 1 && n_probs <= 5) {  // the same probability alone, in the kernel's smallest form
                select<2>(x, probs + i, 1, method, one);
                CHECK(same(one[0], want));
            }
        }
    }
}

// ---- (b) ---------------------------------------------------------------------------------------------------------------------
static uint64_t check_small() {
    const double alpha[5] = {-1.5, -0.0, 0.0, 2.25, std::nan("")}, probs[5] = {0.0, 0.1, 0.5, 0.9, 1.0};
    uint64_t n_checked = 0;
    for (uint32_t len = 0; len <= 7; len++) {
        uint32_t total = 1;
        for (uint32_t i = 0; i < len; i++) total *= 5;
        for (uint32_t code = 0; code < total; code++) {
            std::vector<double> x(len);
            for (uint32_t i = 0, c = code; i < len; i++, c /= 5) x[i] = alpha[c % 5];
            check_series(x, probs, 5);
            n_checked++;
        }
    }
    return n_checked;
}

// ---- (c) ---------------------------------------------------------------------------------------------------------------------
static uint64_t check_random() {
    std::mt19937_64 rng(20240611);
    uint64_t n_checked = 0;
    for (int it = 0; it < 10000; it++) {
        const uint32_t len = 1 + (uint32_t)(rng() % 400), low = 1 + (uint32_t)(rng() % 14);  // bits the keys differ in
        const uint64_t prefix = quantile_key(it % 3 == 0 ? -1234.5678 : it % 3 == 1 ? 3.0e-5 : 7.0e11) & ~(((uint64_t)1 << 20) - 1);
        const uint32_t shift = (uint32_t)(rng() % 6);
        std::vector<double> x(len);
        for (double& e : x) e = rng() % 11 == 0 ? std::nan("") : quantile_unkey(prefix | ((rng() & (((uint64_t)1 << low) - 1)) << shift));
        if (it % 50 == 0) x[rng() % len] = -x[0];  // a sign change: the keys differ in their top bit
        double probs[QUANTILE_MAX_PROBS];
        const uint32_t n_probs = it % 4 == 0 ? 1 : 1 + (uint32_t)(rng() % QUANTILE_MAX_PROBS);
        for (uint32_t i = 0; i < n_probs; i++) probs[i] = (double)(rng() % 1001) / 1000.0;
        check_series(x, probs, n_probs);
        n_checked++;
    }
    return n_checked;
}

// ---- (d) ---------------------------------------------------------------------------------------------------------------------
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
static uint64_t check_plan_case(Geo& G, const std::vector<dcdf_cube>& cubes, bool node_wise, uint64_t cap_bytes) {
    G.g.leaves = G.leaves.data();
    const PlanRaster& g = G.g;
    const size_t nq = cubes.size();
    std::vector<uint64_t> base(nq), plane(nq);
    std::vector<dcdf_cube> nc(nq);
    uint64_t at = 0, volume = 0;
    for (size_t q = 0; q < nq; q++) {
        nc[q] = norm_cube(cubes[q]);
        plane[q] = cube_cells(nc[q]) ? (uint64_t)(nc[q].bottom - nc[q].top) * (nc[q].right - nc[q].left) : 0;
        base[q] = at + 3;
        at = base[q] + 2 * plane[q];  // (two planes a cube)
        volume += cube_cells(nc[q]);
    }
    QuantilePlan P;
    CHECK(plan_quantile_time(g, cubes.data(), nq, base.data(), cap_bytes, node_wise, 64, P) == DCDF_OK);
    DecodePlan D;  // the decode of the cubes themselves: the same cells of each kind
    std::vector<uint64_t> dbase(nq, 0);
    CHECK(plan_decode(g, cubes.data(), nq, dbase.data(), node_wise, 64, D) == DCDF_OK);
    for (int k = 0; k < 3; k++) CHECK(P.stats[k] == D.stats[k]);
    CHECK(P.stats[0] + P.stats[1] + P.stats[2] == volume);
    std::vector<std::vector<uint8_t>> seen(nq);
    for (size_t q = 0; q < nq; q++) seen[q].assign(plane[q], 0);
    size_t a_col = 0, a_unit = 0, a_item = 0, a_const = 0;
    uint64_t records = 0;
    for (const QuantileBand& b : P.bands) {
        CHECK(b.col0 == a_col && b.unit0 == a_unit && b.item0 == a_item && b.const0 == a_const && b.col1 > b.col0);
        a_col = b.col1, a_unit = b.unit1, a_item = b.item1, a_const = b.const1;
        uint64_t used = 0, big = 0, decoded = 0;
        for (size_t i = b.col0; i < b.col1; i++) {
            const QuantileCol& c = P.cols[i];
            CHECK(c.src == used && c.nt > 0 && c.rows > 0 && c.cols > 0);  // the columns' slabs one after the other
            used += (uint64_t)c.nt * c.rows * c.cols;
            big = std::max(big, (uint64_t)c.rows * c.cols);
            size_t q = 0;
            while (q < nq && !(plane[q] && c.o_off >= base[q] && c.o_off < base[q] + plane[q])) q++;
            CHECK(q < nq);
            const dcdf_cube& cu = nc[q];
            const uint32_t wc = cu.right - cu.left;
            CHECK(c.sr == wc && c.psz == plane[q] && c.nt == cu.end - cu.start);
            const uint64_t p = c.o_off - base[q];
            const uint32_t pr = (uint32_t)(p / wc), pc = (uint32_t)(p % wc), r0 = cu.top + pr, c0 = cu.left + pc;
            CHECK(pc + c.cols <= wc && pr + c.rows <= cu.bottom - cu.top);
            const uint32_t ti = r0 / g.tile, tj = c0 / g.tile;
            CHECK((r0 + c.rows - 1) / g.tile == ti && (c0 + c.cols - 1) / g.tile == tj);  // inside one leaf's place
            for (uint32_t r = 0; r < c.rows; r++)
                for (uint32_t cc = 0; cc < c.cols; cc++) {
                    uint8_t& s = seen[q][(uint64_t)(pr + r) * wc + pc + cc];
                    CHECK(s == 0);  // exactly one column
                    s = 1;
                }
            // the table: from the cube's first instant, a new entry exactly at every segment boundary, the leaf's own encoding
            CHECK(c.nseg == (cu.end - 1) / g.cs - cu.start / g.cs + 1 && c.seg0 + c.nseg <= P.segs.size());
            for (uint32_t s = 0; s < c.nseg; s++) {
                const QuantileSeg& e = P.segs[c.seg0 + s];
                const uint32_t seg = cu.start / g.cs + s;
                CHECK(e.t0 == (s == 0 ? 0u : seg * g.cs - cu.start) && e.t0 < c.nt);
                const PlanLeaf& L = g.leaves[((uint64_t)seg * g.nti + ti) * g.ntj + tj];
                CHECK(e.enc == L.enc && e.fbits == L.fbits);
            }
            records += c.nseg;
        }
        CHECK(big == b.max_cells && used <= P.slab_max);
        CHECK(used * sizeof(int64_t) <= cap_bytes || b.col1 - b.col0 == 1);
        // what the band's decode writes: inside [0, used), and as many cells as the slab has
        for (size_t i = b.unit0; i < b.unit1; i++) {
            const BulkUnit& u = P.units[i];
            const uint64_t nt = u.t1 - u.t0, rows = u.bottom - u.top, cols = u.right - u.left;
            CHECK(nt && rows && cols && u.out_off + (nt - 1) * u.out_st + (rows - 1) * u.out_sr + cols <= used);
            decoded += nt * rows * cols;
        }
        for (size_t i = b.item0; i < b.item1; i++) {
            const WinItem& w = P.items[i];
            const uint64_t rows = w.bottom - w.top, cols = w.right - w.left;
            CHECK(rows && cols && w.out_off + (rows - 1) * w.out_sr + cols <= used);
            decoded += rows * cols;
        }
        for (size_t i = b.const0; i < b.const1; i++) {
            const ConstPiece& k = P.consts[i];
            const uint64_t nt = k.le - k.ls;
            CHECK(nt && k.rows && k.cols && k.out_off + (nt - 1) * k.out_st + (uint64_t)(k.rows - 1) * k.out_sr + k.cols <= used);
            decoded += nt * k.rows * k.cols;
        }
        CHECK(decoded == used);
    }
    CHECK(a_col == P.cols.size() && a_unit == P.units.size() && a_item == P.items.size() && a_const == P.consts.size());
    for (size_t q = 0; q < nq; q++)
        for (uint8_t s : seen[q]) CHECK(s == 1);  // every cell of every cube
    return records + P.bands.size();
}
static uint64_t check_plan() {
    uint64_t records = 0, bands_small = 0;
    for (int geo = 0; geo < 4; geo++) {
        Geo G = geo < 3 ? plain(geo) : tiled();
        const uint32_t T = G.g.T, R = G.g.R, C = G.g.C;
        const dcdf_cube inner = geo < 3 ? dcdf_cube{1, 19, 33, 99, 63, 193} : dcdf_cube{1, 19, 5, 39, 20, 90};
        std::vector<dcdf_cube> cubes = {{0, T, 0, R, 0, C}, {T - 2, T - 1, R / 2, R / 2 + 1, C - 1, C}, {4, 4, 0, R, 0, C}, inner, {0, T, 7, 7, 1, C},
                                        {inner.end, inner.start, inner.bottom, inner.top, inner.right, inner.left}};
        std::vector<dcdf_cube> rev(cubes.rbegin(), cubes.rend());
        for (int node_wise = 0; node_wise < 2; node_wise++)
            // a cap below one 64 x 64 part (a column alone), one that cuts rows only, one that cuts nothing, the default
            for (uint64_t cap : {(uint64_t)1000, (uint64_t)20 * 64 * 96 * 8, (uint64_t)20 * 96 * 96 * 8 * 2, (uint64_t)64 << 20}) {
                const uint64_t n = check_plan_case(G, cubes, node_wise != 0, cap);
                records += n + check_plan_case(G, rev, node_wise != 0, cap);
                if (cap == 1000) bands_small += n;
            }
    }
    CHECK(bands_small > 100);
    return records;
}

// ---- (e) ---------------------------------------------------------------------------------------------------------------------
static uint64_t check_ranks() {
    uint64_t n_checked = 0;
    for (uint32_t n = 1; n <= 130; n++)
        for (uint32_t num = 0; num <= 4; num++) {  // p = num / 4: (n - 1) p is exact
            const uint32_t j = (n - 1) * num / 4, rem = (n - 1) * num % 4, j1 = std::min(j + 1, n - 1);
            for (int method = 0; method < 4; method++) {
                const QuantileRank r = quantile_rank(n, num / 4.0, method);
                CHECK(r.j == j && r.j1 == j1 && r.g == rem / 4.0);
                const uint32_t want = method == 0 ? 1u : method == 1 ? (rem ? 2u : 1u) : method == 2 ? (rem < 2 ? 1u : rem > 2 ? 2u : j % 2 == 0 ? 1u : 2u)
                                                                                                     : (rem ? 3u : 1u);
                CHECK(r.need == want);
                n_checked++;
            }
        }
    double bad[3] = {0.5, std::nan(""), 0.5};
    CHECK(quantile_args_ok(bad, 1, 0) && !quantile_args_ok(bad, 2, 0) && !quantile_args_ok(bad, 0, 0) && !quantile_args_ok(bad, 17, 0));
    CHECK(!quantile_args_ok(bad, 1, 4) && !quantile_args_ok(bad, 1, -1) && !quantile_args_ok(nullptr, 1, 0));
    bad[1] = 1.5;
    CHECK(!quantile_args_ok(bad, 2, 3));
    bad[1] = -1e-300;
    CHECK(!quantile_args_ok(bad, 2, 3));
    return n_checked;
}

int main() {
    std::printf("ok keys %" PRIu64 "\n", check_keys());
    std::printf("ok ranks %" PRIu64 "\n", check_ranks());
    std::printf("ok small %" PRIu64 "\n", check_small());
    std::printf("ok random %" PRIu64 "\n", check_random());
    std::printf("ok plan %" PRIu64 "\n", check_plan());
    return 0;
}
