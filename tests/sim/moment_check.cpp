// Stand-alone host program over dcdf_amd/csrc/k2r_moment.h and plan_reduce_time_groups of k2r_plan.h (TEST INFRASTRUCTURE ONLY),
// built with -fsanitize=address,undefined by tests/test_moments_host.py.
//
// Without an argument: the step, the store / load at a change of group and the finish (moment_group_step, moment_store,
// moment_finish: what the fold kernel and the finishing kernel run per cell).  For every label series of up to 8 instants over
// the labels 0, 1, 2 and GROUP_NONE, and for the label-less form (no label array, one group), at every cut of the series into
// consecutive pieces: the pieces stepped one after the other through planes that hold the initial state equal a model written
// apart from the header -- per group, a plain loop with branches over the group's instants --, bit for bit, for both ddof, with
// the set of requested statistics changing from series to series (COUNT in its output plane or in scratch); nothing outside the
// cell's elements is touched.  Prints "ok cuts <count>".
//
// With the name of a file of cases: prints every list of plan_reduce_time_groups as the moments' entry points upload it, in
// tests/sim/group_check.cpp's format (the plan is the grouped reduce's as it is).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_moment.h"
#include "../../dcdf_amd/csrc/k2r_plan.h"

using namespace k2r;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- the step --------------------------------------------------------------------------------------------------------------------
constexpr uint32_t N_GROUPS = 3, LEN = 8;
constexpr uint64_t GSZ = 3, CELL = 1, PSZ = N_GROUPS * GSZ;  // group planes of three cells, the middle one used
constexpr double SENT = -77.25;
// instant i's value: a large level with small differences (the unshifted sums would lose them), one NaN, and values far from the
// level, so that which value comes first in a group -- its K -- shows in the bits
static const double XS[LEN] = {1e6, 1e6 + 1e-3, NAN, 1e6 - 2e-3, 3.5, 1e6 + 0.5, -7.25, 1e6 + 1e-3};

// the model, written apart: group g's instants (label == g; without labels every instant) in order
static void model(const uint32_t* lab, uint32_t len, uint32_t g, uint32_t ddof, double (&w)[4]) {
    double c = 0.0, K = NAN, s1 = 0.0, s2 = 0.0;
    for (uint32_t i = 0; i < len; i++) {
        if ((lab && lab[i] != g) || std::isnan(XS[i])) continue;
        if (c == 0.0) K = XS[i];
        const volatile double d = XS[i] - K;
        const volatile double p = d * d;  // (volatile: the product is rounded before it is added)
        s1 = s1 + d;
        s2 = s2 + p;
        c += 1.0;
    }
    w[0] = c;
    w[1] = w[2] = w[3] = NAN;
    if (c == 0.0) return;
    const volatile double m = s1 / c;
    const volatile double sm = s1 * m;
    double q = s2 - sm;
    if (q < 0.0) q = 0.0;
    w[1] = K + m;
    if (c > (double)ddof) {
        w[2] = q / (c - (double)ddof);
        w[3] = std::sqrt(w[2]);
    }
}
// the instants [a, b) of one cell through its planes, as a piece of the plan runs them: MomentCell of k2r_raster_region.hip
static void piece(const uint16_t* lab, uint32_t a, uint32_t b, uint32_t n_groups, const MomentPlanes& P) {
    MomentRun st = moment_run_init();
    for (uint32_t i = a; i < b; i++) moment_group_step(st, P, moment_label(lab, i), n_groups, XS[i]);
    moment_store(st, P);
}
// one series at one cut; lab == nullptr: the label-less form
static void one_case(const uint16_t* lab, const uint32_t* lab32, uint32_t len, uint32_t cuts, uint32_t ops) {
    const uint32_t n_groups = lab ? N_GROUPS : 1u, n_out = popc32(ops), n_scr = popc32(MS_ALL & ~ops);
    const uint64_t psz = n_groups * GSZ;
    double dst[4 * PSZ], scr[4 * PSZ + 1];
    for (double& x : dst) x = SENT;
    for (double& x : scr) x = SENT;
    // k_moment_fill, into this cell's elements alone
    const MomentPlanes P = moment_planes(dst, scr, ops, CELL, CELL, psz, GSZ);
    const MomentState s0 = moment_init();
    for (uint32_t g = 0; g < n_groups; g++) {
        P.p_c[g * GSZ] = s0.c;
        P.p_k[g * GSZ] = s0.K;
        P.p_s1[g * GSZ] = s0.s1;
        P.p_s2[g * GSZ] = s0.s2;
    }
    for (uint32_t a = 0; a < len;) {
        uint32_t b = a + 1;
        while (b < len && !((cuts >> (b - 1)) & 1u)) b++;
        piece(lab, a, b, n_groups, P);
        a = b;
    }
    for (uint32_t ddof = 0; ddof <= 1; ddof++) {
        for (uint32_t g = 0; g < n_groups; g++) {
            // k_moment_finish
            double o[4], want[4];
            moment_finish(MomentState{P.p_c[g * GSZ], P.p_k[g * GSZ], P.p_s1[g * GSZ], P.p_s2[g * GSZ]}, ddof, o);
            for (uint32_t A = MO_MEAN; A <= MO_STD; A <<= 1)
                if (ops & A) moment_plane(A, dst, scr, ops, CELL, CELL, psz)[g * GSZ] = o[A == MO_MEAN ? 1 : A == MO_VAR ? 2 : 3];
            model(lab32, len, g, ddof, want);
            uint32_t plane = 0;
            for (uint32_t b = 0; b < 4; b++) {
                if (!(ops & (1u << b))) continue;
                const double* const p = dst + (uint64_t)plane++ * psz + g * GSZ;  // the planes in the order count, mean, var, std
                CHECK(same_bits(p[CELL], want[b]));
                CHECK(p[0] == SENT && p[2] == SENT);
            }
            if (!(ops & MO_COUNT)) CHECK(same_bits(scr[CELL + g * GSZ], want[0]));  // an unrequested COUNT: the first scratch plane
        }
    }
    for (uint64_t e = n_out * psz; e < 4 * PSZ; e++) CHECK(dst[e] == SENT);
    for (uint64_t e = n_scr * psz; e < 4 * PSZ + 1; e++) CHECK(scr[e] == SENT);
    for (uint32_t s = 0; s < n_scr; s++)
        for (uint32_t g = 0; g < n_groups; g++) CHECK(scr[s * psz + g * GSZ] == SENT && scr[s * psz + g * GSZ + 2] == SENT);
}
static uint64_t check_cuts() {
    uint64_t n = 0;
    const uint16_t alphabet[4] = {0u, 1u, 2u, (uint16_t)GROUP_NONE};
    for (uint32_t len = 0; len <= LEN; len++) {
        const uint32_t n_series = 1u << (2 * len), n_cuts = len ? 1u << (len - 1) : 1u;  // bit i of cuts: a cut between instants i and i + 1
        for (uint32_t code = 0; code < n_series; code++) {
            uint16_t lab[LEN] = {};
            uint32_t lab32[LEN] = {};
            for (uint32_t i = 0; i < len; i++) lab32[i] = lab[i] = alphabet[(code >> (2 * i)) & 3u];
            const uint32_t ops = 1u + code % 15u;
            for (uint32_t cuts = 0; cuts < n_cuts; cuts++, n++) one_case(lab, lab32, len, cuts, ops);
        }
        for (uint32_t ops = 1; ops <= MO_ALL; ops++)
            for (uint32_t cuts = 0; cuts < n_cuts; cuts++, n++) one_case(nullptr, nullptr, len, cuts, ops);
    }
    // the properties the header states
    MomentState s = moment_init();
    double o[4];
    for (int i = 0; i < 5; i++) moment_step(s, 0.1);
    moment_finish(s, 1, o);
    CHECK(same_bits(o[2], 0.0) && same_bits(o[3], 0.0) && same_bits(o[1], 0.1) && o[0] == 5.0);
    s = moment_init();
    moment_step(s, 42.0);
    moment_finish(s, 1, o);
    CHECK(o[0] == 1.0 && o[1] == 42.0 && std::isnan(o[2]) && std::isnan(o[3]));
    moment_finish(s, 0, o);
    CHECK(same_bits(o[2], 0.0) && same_bits(o[3], 0.0));
    moment_finish(moment_init(), 0, o);
    CHECK(o[0] == 0.0 && std::isnan(o[1]) && std::isnan(o[2]) && std::isnan(o[3]));
    for (double v : {2.0, 3.0, 1e-300, 1e300, 0.1, 4.0, 1e-320, 0.0}) CHECK(same_bits(moment_sqrt(v), std::sqrt(v)));
    return n;
}

// ---- the plan --------------------------------------------------------------------------------------------------------------------
static void put(const char* tag, std::initializer_list<uint64_t> v) {
    std::printf("%s", tag);
    for (uint64_t x : v) std::printf(" %" PRIu64, x);
    std::printf("\n");
}
static void put_fold(const char* tag, const GroupFold& f) {
    put(tag, {f.nt, f.rows, f.cols, f.sr, f.init, (uint64_t)(int64_t)f.enc, f.fbits, f.elided, f.src, f.o_off, f.s_off, f.psz, f.lab, f.gsz});
}
static int dump_plans(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    PlanRaster g{};
    uint32_t step, n_groups;
    uint64_t slab_cap;
    while (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu32, &g.T, &g.R, &g.C, &g.tile, &g.cs,
                       &step, &slab_cap, &n_groups) == 8) {
        if (!g.T || !g.R || !g.C || !g.tile || !g.cs || !n_groups) return 3;
        g.nti = (g.R + g.tile - 1) / g.tile;
        g.ntj = (g.C + g.tile - 1) / g.tile;
        size_t n_leaves, nq;
        if (std::fscanf(f, "%zu", &n_leaves) != 1 || n_leaves != (size_t)((g.T + g.cs - 1) / g.cs) * g.nti * g.ntj) return 3;
        std::vector<PlanLeaf> leaves(n_leaves);
        for (PlanLeaf& L : leaves) {
            uint32_t el, ok;
            if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &L.row0, &L.col0, &L.enc, &L.fbits, &el, &ok) != 6) return 3;
            L.elided = (uint8_t)el;
            L.bulk_ok = (uint8_t)ok;
        }
        g.leaves = leaves.data();
        if (std::fscanf(f, "%zu", &nq) != 1 || nq > 100000) return 3;
        std::vector<dcdf_cube> cubes(nq);
        std::vector<uint64_t> base(nq), sbase(nq), loff(nq);
        for (size_t q = 0; q < nq; q++) {
            dcdf_cube& c = cubes[q];
            if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64, &c.start, &c.end, &c.top,
                            &c.bottom, &c.left, &c.right, &base[q], &sbase[q], &loff[q]) != 9)
                return 3;
        }
        std::printf("case\n");
        if (plan_bounds(g, cubes.data(), nq) != DCDF_OK) return 3;
        GroupPlan P(slab_cap);
        std::printf("groups %d\n", plan_reduce_time_groups(g, cubes.data(), nq, loff.data(), n_groups, base.data(), sbase.data(), step == 64, P));
        for (const GroupUnit& u : P.units)
            put("unit", {u.chunk, u.t0, u.t1, u.rr, u.rc, u.top, u.bottom, u.left, u.right, u.sr, u.init, u.o_off, u.s_off, u.psz, u.lab, u.gsz});
        for (const GroupFold& c : P.cfolds) put_fold("cfold", c);
        for (const GroupFold& w : P.walk.folds) put_fold("wfold", w);
        for (const WinItem& i : P.walk.items) put("item", {i.chunk, i.inst, i.top, i.bottom, i.left, i.right, i.out_sr, i.out_off});
        for (const Slab& s : P.walk.slabs) put("slab", {s.item0, s.item1, s.fold0, s.fold1});
        put("slab_max", {P.walk.slab_max, P.walk.fold_nt});
        for (const SegRange& r : P.ranges) put("range", {r.unit0, r.unit1, r.const0, r.const1, r.slab0, r.slab1});
        for (const MeanPiece& m : P.means) put("mean", {m.o_off, m.s_off, m.psz});
        put("stats", {P.stats[0], P.stats[1], P.stats[2]});
        std::printf("end\n");
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2) return dump_plans(argv[1]);
    if (argc != 1) return 2;
    std::printf("ok cuts %" PRIu64 "\n", check_cuts());
    return 0;
}
