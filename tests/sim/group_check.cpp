// Stand-alone host program over dcdf_amd/csrc/k2r_group.h and plan_reduce_time_groups of k2r_plan.h (TEST INFRASTRUCTURE ONLY),
// built with -fsanitize=address,undefined by tests/test_reduce_time_groups_host.py.
//
// Without an argument: the merge-on-change step (group_step / group_merge, what the fold kernel runs per cell).  For every label
// series of up to 8 instants over the labels 0, 1 and GROUP_NONE, every cut of the series into consecutive parts and several sets
// of statistics: the parts stepped one after the other through planes that were filled with the identities equal a model written
// apart from group_step -- per group, the plain scan of its sub-series --, bit for bit, and nothing outside the cell's elements
// is touched.  The values make the order of a sum observable.  Prints "ok cuts <count>".
//
// With "--gather": the label gather of the grouped calls (gather_time_labels) over a batch of five cubes -- with cells, without
// instants, with zero rows, with reversed bounds, with cells --, each cube's labels at its own offset of an exactly sized array,
// against a naive loop; the labels of a cube without cells lie outside the array and must not be read.  Null labels yield nothing.
// Prints "ok gather".
//
// With the name of a file of cases: prints every list of plan_reduce_time_groups as the entry point would upload it.
//   case:  T R C tile cs  step(64 | 32)  slab_cap  n_groups
//          n_leaves, then per leaf: row0 col0 enc fbits elided bulk_ok
//          nq, then per cube: start end top bottom left right  base sbase loff
//   output: "case", "groups <code>", then one line per record: "<list> <field> ..." in the struct's field order, "stats b w c", "end".
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- the step --------------------------------------------------------------------------------------------------------------------
constexpr uint32_t N_GROUPS = 2, LEN = 8;
// instant i's value: sums of these depend on the order (2^53 absorbs a 1.0 that follows it, not one that precedes it); one NaN
static const double XS[LEN] = {1.0, 9007199254740992.0, 1.0, -9007199254740992.0, NAN, 0.5, -3.0, 9007199254740993.0 * 2.0};

// the instants [a, b) of one cell through its planes, as a piece of the plan runs them: GroupCell of k2r_raster_region.hip
static void piece(const uint32_t* lab, uint32_t a, uint32_t b, uint32_t ops, double* dst, double* scr, uint64_t o_off, uint64_t s_off, uint64_t psz,
                  uint64_t gsz) {
    const uint32_t live = reduce_live(ops);
    GroupPlanes P;
    P.p_min = live & RA_MIN ? reduce_plane(RA_MIN, dst, scr, ops, o_off, s_off, psz) : nullptr;
    P.p_max = live & RA_MAX ? reduce_plane(RA_MAX, dst, scr, ops, o_off, s_off, psz) : nullptr;
    P.p_sum = live & RA_SUM ? reduce_plane(RA_SUM, dst, scr, ops, o_off, s_off, psz) : nullptr;
    P.p_cnt = live & RA_COUNT ? reduce_plane(RA_COUNT, dst, scr, ops, o_off, s_off, psz) : nullptr;
    P.gsz = gsz;
    GroupState st = group_init();
    for (uint32_t i = a; i < b; i++) group_step(st, P, lab[i], N_GROUPS, XS[i]);
    group_merge(st, P);
}
static uint64_t check_cuts() {
    uint64_t n = 0;
    constexpr uint64_t GSZ = 3, CELL = 1, PSZ = N_GROUPS * GSZ;  // group planes of three cells, the middle one used
    constexpr double SENT = -77.25;
    const uint32_t alphabet[3] = {0u, 1u, GROUP_NONE};
    const uint32_t op_sets[] = {RA_ALL | ROP_MEAN, ROP_MEAN, RA_SUM, RA_MIN | RA_COUNT, RA_MAX};
    for (uint32_t len = 0; len <= LEN; len++) {
        uint32_t n_series = 1;
        for (uint32_t i = 0; i < len; i++) n_series *= 3u;
        for (uint32_t code = 0; code < n_series; code++) {
            uint32_t lab[LEN] = {};
            for (uint32_t i = 0, c = code; i < len; i++, c /= 3u) lab[i] = alphabet[c % 3u];
            // the model: per group, a plain scan of the instants that carry its label
            double w_min[N_GROUPS], w_max[N_GROUPS], w_sum[N_GROUPS], w_cnt[N_GROUPS];
            for (uint32_t g = 0; g < N_GROUPS; g++) {
                w_min[g] = w_max[g] = NAN;
                w_sum[g] = w_cnt[g] = 0.0;
                for (uint32_t i = 0; i < len; i++) {
                    if (lab[i] != g || std::isnan(XS[i])) continue;
                    w_sum[g] = w_sum[g] + XS[i];
                    w_cnt[g] += 1.0;
                    w_min[g] = std::isnan(w_min[g]) || XS[i] < w_min[g] ? XS[i] : w_min[g];
                    w_max[g] = std::isnan(w_max[g]) || XS[i] > w_max[g] ? XS[i] : w_max[g];
                }
            }
            for (uint32_t ops : op_sets) {
                if (ops != (RA_ALL | ROP_MEAN) && (code % 5u) != 0) continue;  // (the other op sets on a fifth of the series)
                const uint32_t live = reduce_live(ops), n_out = popc32(ops), n_scr = popc32(live & ~ops);
                const uint32_t n_cuts = len ? 1u << (len - 1) : 1u;  // bit i: a cut between instants i and i + 1
                for (uint32_t cuts = 0; cuts < n_cuts; cuts++) {
                    std::vector<double> dst(n_out * PSZ, SENT), scr(n_scr * PSZ + 1, SENT);
                    // k_group_fill's identities, into this cell's elements alone
                    for (uint32_t A = RA_MIN; A <= RA_COUNT; A <<= 1)
                        if (live & A)
                            for (uint32_t g = 0; g < N_GROUPS; g++)
                                reduce_plane(A, dst.data(), scr.data(), ops, CELL, CELL, PSZ)[g * GSZ] = A & (RA_MIN | RA_MAX) ? NAN : 0.0;
                    for (uint32_t a = 0; a < len;) {
                        uint32_t b = a + 1;
                        while (b < len && !((cuts >> (b - 1)) & 1u)) b++;
                        piece(lab, a, b, ops, dst.data(), scr.data(), CELL, CELL, PSZ, GSZ);
                        a = b;
                    }
                    for (uint32_t g = 0; g < N_GROUPS; g++) {
                        const double want[4] = {w_min[g], w_max[g], w_sum[g], w_cnt[g]};
                        for (uint32_t b = 0; b < 4; b++) {
                            if (!(live & (1u << b))) continue;
                            const double* const p = reduce_plane(1u << b, dst.data(), scr.data(), ops, 0, 0, PSZ) + g * GSZ;
                            CHECK(same_bits(p[CELL], want[b]));
                            CHECK(p[0] == SENT && p[2] == SENT);
                        }
                    }
                    CHECK(scr[n_scr * PSZ] == SENT);
                    n++;
                }
            }
        }
    }
    return n;
}

// ---- the label gather ------------------------------------------------------------------------------------------------------------
static void check_gather() {
    //                       start end top bottom left right
    const dcdf_cube cubes[5] = {{2, 7, 0, 3, 1, 4}, {4, 4, 0, 3, 0, 3}, {1, 5, 2, 2, 0, 3}, {9, 6, 5, 1, 8, 2}, {0, 1, 0, 1, 0, 1}};
    const uint64_t offset[5] = {4, 9, 1000000, 0, 3};  // cube 3's three labels, cube 4's one, cube 0's five; cube 2's are nowhere
    std::vector<uint16_t> labels(9);
    for (size_t i = 0; i < labels.size(); i++) labels[i] = (uint16_t)(100 + 7 * i);
    labels[8] = GROUP_NONE;
    // the naive loop: the cubes that have cells, their |end - start| labels each, in batch order
    std::vector<uint64_t> want_off(5, 0);
    std::vector<uint16_t> want;
    for (size_t q = 0; q < 5; q++) {
        const dcdf_cube& c = cubes[q];
        const uint64_t nt = c.start < c.end ? c.end - c.start : c.start - c.end, rows = c.top < c.bottom ? c.bottom - c.top : c.top - c.bottom,
                       cols = c.left < c.right ? c.right - c.left : c.left - c.right;
        if (nt * rows * cols == 0) continue;
        want_off[q] = want.size();
        for (uint64_t i = 0; i < nt; i++) want.push_back(labels[offset[q] + i]);
    }
    CHECK(want.size() == 9 && want_off[3] == 5 && want_off[4] == 8);
    std::vector<uint64_t> loff(3, 77);  // (what an earlier call left)
    std::vector<uint16_t> lab(2, 5);
    gather_time_labels(cubes, 5, labels.data(), offset, loff, lab);
    CHECK(loff == want_off && lab == want);
    gather_time_labels(cubes, 5, nullptr, nullptr, loff, lab);
    CHECK(loff == std::vector<uint64_t>(5, 0) && lab.empty());
    gather_time_labels(cubes, 0, labels.data(), offset, loff, lab);
    CHECK(loff.empty() && lab.empty());
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
    if (argc == 2 && !std::strcmp(argv[1], "--gather")) {
        check_gather();
        std::printf("ok gather\n");
        return 0;
    }
    if (argc == 2) return dump_plans(argv[1]);
    if (argc != 1) return 2;
    std::printf("ok cuts %" PRIu64 "\n", check_cuts());
    return 0;
}
