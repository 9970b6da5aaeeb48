// Stand-alone host program over dcdf_amd/csrc/k2r_regress.h (TEST INFRASTRUCTURE ONLY), built with -fsanitize=address,undefined by
// tests/test_regress_host.py.
//
// The step and the finish (regress_step, regress_finish) with the state stored and loaded whole between the pieces of a series.
// For every series of up to 8 instants over three kinds of value -- a large level with a small difference, a value far from the
// level, NaN --, against a fixed regressor, at every cut of the series into consecutive pieces: the pieces stepped one after the
// other, the seven doubles of the state written to an array behind each piece and read back before the next, equal a model written
// apart from the header -- a plain loop with branches over the series --, bit for bit; nothing outside the seven elements is
// touched.  Then the properties the header states.  Prints "ok cuts <count>".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dcdf_amd/csrc/k2r_regress.h"

using namespace k2r;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

constexpr uint32_t LEN = 8;
constexpr double SENT = -77.25;
// the three kinds of value (which one comes first -- K -- shows in the bits), and instant i's regressor value
static const double KINDS[3] = {1e6 + 1e-3, -2.5, NAN};
static const double ES[LEN] = {0.0, 1.5, -2.25, 3.0, 1000.125, 5.5, -7.0, 0.3};

// the model, written apart
static void model(const double* xs, uint32_t len, double (&w)[4]) {
    double c = 0.0, K = NAN, sy = 0.0, syy = 0.0, se = 0.0, see = 0.0, sey = 0.0;
    for (uint32_t i = 0; i < len; i++) {
        if (std::isnan(xs[i])) continue;
        if (c == 0.0) K = xs[i];
        const volatile double d = xs[i] - K;
        const volatile double dd = d * d, ee = ES[i] * ES[i], ed = ES[i] * d;  // (volatile: a product is rounded before it is added)
        sy = sy + d;
        syy = syy + dd;
        se = se + ES[i];
        see = see + ee;
        sey = sey + ed;
        c += 1.0;
    }
    w[0] = c;
    w[1] = w[2] = w[3] = NAN;
    if (c < 2.0) return;
    const volatile double me = se / c, my = sy / c;
    const volatile double pe = se * me, py = sy * my, pc = se * my;
    double See = see - pe, Syy = syy - py;
    const double Sey = sey - pc;
    if (See < 0.0) See = 0.0;
    if (Syy < 0.0) Syy = 0.0;
    if (!(See > 0.0)) return;
    w[1] = Sey / See;
    const volatile double at0 = K + my, lift = w[1] * me;
    w[2] = at0 - lift;
    if (Syy > 0.0) {
        const volatile double p = See * Syy;
        const double r = Sey / std::sqrt(p);
        w[3] = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
    }
}
// the instants [a, b) through the stored state
static void piece(const double* xs, uint32_t a, uint32_t b, double* st) {
    RegressState s{st[0], st[1], st[2], st[3], st[4], st[5], st[6]};
    for (uint32_t i = a; i < b; i++) regress_step(s, xs[i], ES[i]);
    const double now[7] = {s.c, s.K, s.sy, s.syy, s.se, s.see, s.sey};
    for (int i = 0; i < 7; i++) st[i] = now[i];
}
static uint64_t check_cuts() {
    uint64_t n = 0;
    for (uint32_t len = 0; len <= LEN; len++) {
        uint32_t n_series = 1;
        for (uint32_t i = 0; i < len; i++) n_series *= 3u;
        const uint32_t n_cuts = len ? 1u << (len - 1) : 1u;  // bit i of cuts: a cut between instants i and i + 1
        for (uint32_t code = 0; code < n_series; code++) {
            double xs[LEN] = {};
            for (uint32_t i = 0, c = code; i < len; i++, c /= 3u) xs[i] = KINDS[c % 3u];
            double want[4];
            model(xs, len, want);
            for (uint32_t cuts = 0; cuts < n_cuts; cuts++, n++) {
                double mem[9] = {SENT, 0, 0, 0, 0, 0, 0, 0, SENT};
                const RegressState s0 = regress_init();
                const double first[7] = {s0.c, s0.K, s0.sy, s0.syy, s0.se, s0.see, s0.sey};
                for (int i = 0; i < 7; i++) mem[1 + i] = first[i];
                for (uint32_t a = 0; a < len;) {
                    uint32_t b = a + 1;
                    while (b < len && !((cuts >> (b - 1)) & 1u)) b++;
                    piece(xs, a, b, mem + 1);
                    a = b;
                }
                double o[4];
                regress_finish(RegressState{mem[1], mem[2], mem[3], mem[4], mem[5], mem[6], mem[7]}, o);
                for (int i = 0; i < 4; i++) CHECK(same_bits(o[i], want[i]));
                CHECK(mem[0] == SENT && mem[8] == SENT);
            }
        }
    }
    // the properties the header states
    RegressState s = regress_init();
    double o[4];
    for (int i = 0; i < 5; i++) regress_step(s, 0.1, (double)i - 2.0);
    regress_finish(s, o);
    CHECK(o[0] == 5.0 && same_bits(o[1], 0.0) && same_bits(o[2], 0.1) && std::isnan(o[3]));
    s = regress_init();
    regress_step(s, 42.0, 3.0);
    regress_step(s, NAN, 4.0);
    regress_finish(s, o);
    CHECK(o[0] == 1.0 && std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3]));
    regress_step(s, 43.0, 3.0);  // two values, one regressor value: See == 0
    regress_finish(s, o);
    CHECK(o[0] == 2.0 && std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3]));
    regress_finish(regress_init(), o);
    CHECK(o[0] == 0.0 && std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3]));
    const double qnan = __builtin_nan("");
    for (int i = 1; i < 4; i++) CHECK(same_bits(o[i], qnan));
    s = regress_init();
    for (int i = 0; i < 6; i++) regress_step(s, 7.0 - 2.0 * i, (double)i);  // an exact line
    regress_finish(s, o);
    CHECK(o[0] == 6.0 && o[1] == -2.0 && o[2] == 7.0 && o[3] == -1.0);
    return n;
}

int main(int argc, char**) {
    if (argc != 1) return 2;
    std::printf("ok cuts %" PRIu64 "\n", check_cuts());
    return 0;
}
