// Stand-alone host program over rolling_cell (dcdf_amd/csrc/k2r_rolling.h) (TEST INFRASTRUCTURE ONLY), built with
// -fsanitize=address,undefined by tests/test_rolling_host.py: the cell body of k_rolling_stream against a naive loop that sums
// every window again, on series of up to 8 instants over the four values {3, -2.5, 2^53, NaN}.  The instants lie in three
// segments of different encodings -- float64 with 1 fractional bit, float64 with 4, float32 with 1 --, so one value has another
// stored integer in every segment.  The naive loop works on __int128 (nine values of at most 2^116 at the 2^-63 scale fit) with
// a rounding of its own.  Enumerated:
//   A  every series of 0 .. 8 instants x every window 1 .. 9 x every min_count 1 .. window, SUM, and MEAN where min_count ==
//      window, under two labellings: all one group (one rebuild, then slides only) and i % 2 (a rebuild for every window);
//   B  every label series over {0, 1, none} of 0 .. 8 instants x every window x every min_count, each with 32 series taken at a
//      stride through all 4^n, a different offset for every label series -- runs of slides and rebuilds of every length and place.
// The full product of A's series with B's label series is 2 * 10^10 cell bodies and is not enumerated.  Prints "ok cells <A> <B>".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_rolling.h"

using namespace k2r;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

typedef __int128 i128;

static uint64_t bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}
static const QuantileSeg SEGS[3] = {{0, ENC_F64, 1}, {3, ENC_F64, 4}, {6, ENC_F32, 1}};
static const uint32_t SEG_OF[9] = {0, 0, 0, 1, 1, 1, 2, 2, 2};
static const double VALUE[3] = {3.0, -2.5, 9007199254740992.0};
// the stored integer of symbol s (3 = NaN) at instant t: x * 2^(fbits + 1) + 1
static int64_t stored(uint32_t s, uint32_t t) {
    if (s == 3) return 0;
    return (int64_t)(VALUE[s] * (double)((int64_t)1 << (SEGS[SEG_OF[t]].fbits + 1))) + 1;
}
// v / 2^63 as the nearest double, ties to even
static double rounded(i128 v) {
    const bool neg = v < 0;
    unsigned __int128 m = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    if (m == 0) return 0.0;
    int p = 127;
    while (!((m >> p) & 1)) p--;
    int low = p > 52 ? p - 52 : 0;
    uint64_t q = (uint64_t)(m >> low);
    if (low > 0) {
        const unsigned __int128 rest = m & (((unsigned __int128)1 << low) - 1), half = (unsigned __int128)1 << (low - 1);
        if (rest > half || (rest == half && (q & 1u))) q++;
    }
    const double r = std::ldexp((double)q, low - 63);
    return neg ? -r : r;
}

static uint64_t n_slides = 0, n_rebuilds = 0;
// one (series, labels) under every window, min_count and kind
static uint64_t run(uint32_t n, const uint32_t* sym, const uint32_t* lab, uint32_t n_groups) {
    int64_t ser[8];
    i128 val[8];
    bool ok[8];
    for (uint32_t t = 0; t < n; t++) {
        ser[t] = stored(sym[t], t);
        ok[t] = sym[t] != 3;
        val[t] = ok[t] ? (i128)(VALUE[sym[t]] * 2.0) * ((i128)1 << 62) : 0;  // (x * 2 is an integer)
    }
    uint64_t runs = 0;
    for (uint32_t w = 1; w <= 9; w++) {
        // the tables the planner would make: ends by (label, instant), the CSR
        uint32_t ends[8], start[3] = {0, 0, 0};
        uint32_t k = 0;
        for (uint32_t g = 0; g < n_groups; g++) {
            start[g] = k;
            for (uint32_t t = w - 1; t < n; t++)
                if (lab[t] == g) {
                    if (k > start[g] && ends[k - 1] + 1 == t) n_slides++;
                    else n_rebuilds++;
                    ends[k++] = t;
                }
        }
        start[n_groups] = k;
        for (uint32_t mc = 1; mc <= w; mc++)
            for (int32_t kind = 0; kind < (mc == w ? 2 : 1); kind++) {
                double got[10];
                uint32_t puts = 0, seen = 0;
                rolling_cell(
                    ends, start, n_groups, SEG_OF, SEGS, RW_ALL, w, mc, kind,
                    [&](uint32_t t) {
                        CHECK(t < n);
                        return ser[t];
                    },
                    [&](uint32_t pl, double v) {
                        CHECK(pl < 5 * n_groups && !(seen >> pl & 1u));
                        seen |= 1u << pl;
                        got[pl] = v;
                        puts++;
                    });
                CHECK(puts == 5 * n_groups);
                for (uint32_t g = 0; g < n_groups; g++) {
                    i128 mx = 0, mn = 0;
                    uint32_t amx = 0, amn = 0, valid = 0;
                    for (uint32_t t = w - 1; t < n; t++) {
                        if (lab[t] != g) continue;
                        i128 S = 0;
                        uint32_t c = 0;
                        for (uint32_t u = t + 1 - w; u <= t; u++) S += val[u], c += ok[u];
                        if (c < mc) continue;
                        if (!valid || S > mx) mx = S, amx = t;
                        if (!valid || S < mn) mn = S, amn = t;
                        valid++;
                    }
                    const double nan = std::nan("");
                    double hi = rounded(mx), lo = rounded(mn);
                    if (kind == 1) {
                        volatile double a = hi / (double)w, b = lo / (double)w;
                        hi = a, lo = b;
                    }
                    const double want[5] = {valid ? hi : nan, valid ? (double)amx : nan, valid ? lo : nan, valid ? (double)amn : nan, (double)valid};
                    for (uint32_t s = 0; s < 5; s++)
                        if (bits(got[s * n_groups + g]) != bits(want[s])) {
                            std::printf("FAILED n %u window %u min_count %u kind %d group %u statistic %u: %.17g, want %.17g; series", n, w, mc, kind, g, s,
                                        got[s * n_groups + g], want[s]);
                            for (uint32_t t = 0; t < n; t++) std::printf(" %u/%u", sym[t], lab[t]);
                            std::printf("\n");
                            std::exit(1);
                        }
                }
                runs++;
            }
    }
    return runs;
}

int main() {
    uint64_t a_runs = 0, b_runs = 0;
    for (uint32_t t = 0; t < 9; t++)  // the stored integers decode to the values
        for (uint32_t s = 0; s < 3; s++) {
            const QuantileSeg& G = SEGS[SEG_OF[t]];
            CHECK(reduce_widen(G.enc, G.fbits, stored(s, t)) == VALUE[s]);
        }
    for (uint32_t n = 0; n <= 8; n++) {
        uint32_t sym[8], lab[8];
        // A: every series, one group and i % 2
        for (uint32_t code = 0; code < (1u << (2 * n)); code++) {
            for (uint32_t t = 0; t < n; t++) sym[t] = code >> (2 * t) & 3u;
            for (uint32_t t = 0; t < n; t++) lab[t] = 0;
            a_runs += run(n, sym, lab, 1);
            for (uint32_t t = 0; t < n; t++) lab[t] = t % 2;
            a_runs += run(n, sym, lab, 2);
        }
        // B: every label series over {0, 1, none}, 32 series each (all of them while 4^n <= 32)
        uint32_t n_lab = 1;
        for (uint32_t t = 0; t < n; t++) n_lab *= 3;
        const uint32_t n_ser = 1u << (2 * n), stride = n_ser > 32 ? n_ser / 32 : 1;
        for (uint32_t lc = 0; lc < n_lab; lc++) {
            uint32_t r = lc;
            for (uint32_t t = 0; t < n; t++, r /= 3) lab[t] = r % 3 == 2 ? 0xffffu : r % 3;
            for (uint32_t code = (lc * 2654435761u) % stride; code < n_ser; code += stride) {
                for (uint32_t t = 0; t < n; t++) sym[t] = code >> (2 * t) & 3u;
                b_runs += run(n, sym, lab, 2);
            }
        }
    }
    CHECK(n_slides > 1000 && n_rebuilds > 1000);
    std::printf("ok cells %" PRIu64 " %" PRIu64 "\n", a_runs, b_runs);
    return 0;
}
