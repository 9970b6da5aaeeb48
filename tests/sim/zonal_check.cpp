// Stand-alone host program over dcdf_amd/csrc/k2r_zonal.h and plan_zonal of k2r_plan.h (TEST INFRASTRUCTURE ONLY): the K2R_HD
// arithmetic and the planner of dcdf_raster_zonal_batch, run on a CPU -- built with -fsanitize=address,undefined by
// tests/test_zonal_host.py.  Reads commands from the file named on the command line, prints one line per command (hex words):
//   L a0 .. a5            -> rc bits: zonal_fold + space_round of six int64 counters (rc 0 when the total is no 192-bit integer)
//   S hi lo scale         -> ok l0 .. l5: space_scaled cut into limbs (zonal_limb), ok = zonal_fold of them gives it back
//   K n bits * n          -> per double: its key, and the bits zonal_unkey returns for the key
//   R r0 n label * n      -> n_distinct, then per label its zone slot in the round that starts at rank r0 (ffffffff: none), as
//                            k_bulk_zonal's 256 threads find it: bitmap, zonal_count8, the scan, zonal_prefix8, zonal_rank
//   P T R C tile cs step slab_cap acc_cap wanted n_zones, n_leaves, leaves, nq, cubes with base and moff (plan_check.cpp's layout)
//                         -> "plan rc", then one line per span / batch / unit / cfold / wfold, "max entries span_nt", "stats", "end"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_plan.h"

using namespace k2r;

static void put(const char* tag, std::initializer_list<uint64_t> v) {
    std::printf("%s", tag);
    for (uint64_t x : v) std::printf(" %" PRIu64, x);
    std::printf("\n");
}

static int rank_round(FILE* f) {
    uint32_t r0;
    size_t n;
    if (std::fscanf(f, "%" SCNu32 " %zu", &r0, &n) != 2 || n > 4096) return 3;
    std::vector<uint32_t> lab(4096, ZONAL_NONE);  // thread t owns the cells 16 t .. 16 t + 15
    for (size_t i = 0; i < n; i++)
        if (std::fscanf(f, "%" SCNu32, &lab[i]) != 1 || lab[i] > 0xffffu) return 3;
    std::vector<uint32_t> bm(ZONAL_BM_WORDS, 0u), pre(ZONAL_BM_WORDS, 0u), mine(256);
    for (uint32_t l : lab)
        if (l != ZONAL_NONE) bm[l >> 5] |= 1u << (l & 31u);
    for (uint32_t t = 0; t < 256u; t++) mine[t] = zonal_count8(bm.data(), t);
    uint32_t start = 0;
    for (uint32_t t = 0; t < 256u; t++) {
        zonal_prefix8(bm.data(), pre.data(), t, start);
        start += mine[t];
    }
    std::printf("%x", start);
    for (size_t i = 0; i < n; i++) {
        uint32_t s = 0xffffffffu;
        if (lab[i] != ZONAL_NONE) {
            const uint32_t r = zonal_rank(bm.data(), pre.data(), lab[i]) - r0;
            if (r < ZONAL_ZL) s = r;
        }
        std::printf(" %x", s);
    }
    std::printf("\n");
    return 0;
}

static int plan(FILE* f) {
    PlanRaster g{};
    uint32_t step, wanted, n_zones;
    uint64_t slab_cap, acc_cap;
    if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32, &g.T, &g.R,
                    &g.C, &g.tile, &g.cs, &step, &slab_cap, &acc_cap, &wanted, &n_zones) != 10)
        return 3;
    if (!g.T || !g.R || !g.C || !g.tile || !g.cs || !n_zones) return 3;
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
    std::vector<uint64_t> base(nq), mo(nq);
    for (size_t q = 0; q < nq; q++) {
        dcdf_cube& c = cubes[q];
        if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64, &c.start, &c.end, &c.top, &c.bottom,
                        &c.left, &c.right, &base[q], &mo[q]) != 8)
            return 3;
    }
    if (plan_bounds(g, cubes.data(), nq) != DCDF_OK) return 3;
    ZonalPlan P(slab_cap);
    std::printf("plan %d\n", plan_zonal(g, cubes.data(), nq, base.data(), mo.data(), n_zones, step == 64, acc_cap, wanted, P));
    for (const ZonalSpan& s : P.spans) put("span", {s.acc, s.nt, s.o_off, s.o_zone, s.o_stat});
    for (const ZonalBatch& b : P.batches) put("batch", {b.unit0, b.unit1, b.const0, b.const1, b.slab0, b.slab1, b.span0, b.span1, b.entries});
    for (const ZonalUnit& u : P.units)
        put("unit", {u.chunk, u.t0, u.t1, u.rr, u.rc, u.top, u.bottom, u.left, u.right, u.m_sr, u.a_st, u.acc, u.m_off});
    for (const ZonalFold& c : P.cfolds) put("cfold", {c.nt, c.rows, c.cols, c.m_sr, (uint64_t)(int64_t)c.enc, c.fbits, c.elided, c.a_st, c.src, c.acc, c.m_off});
    for (const ZonalFold& c : P.walk.folds)
        put("wfold", {c.nt, c.rows, c.cols, c.m_sr, (uint64_t)(int64_t)c.enc, c.fbits, c.elided, c.a_st, c.src, c.acc, c.m_off});
    for (const Slab& s : P.walk.slabs) put("slab", {s.item0, s.item1, s.fold0, s.fold1});
    put("max", {P.entries_max, P.span_nt, P.walk.items.size()});
    put("stats", {P.stats[0], P.stats[1], P.stats[2]});
    std::printf("end\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[4];
    while (std::fscanf(f, "%3s", cmd) == 1) {
        if (cmd[0] == 'L') {
            int64_t l[6];
            for (int64_t& x : l)
                if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
            U192 v;
            const bool ok = zonal_fold(l, v);
            const double d = ok ? space_round(v) : 0.0;
            uint64_t b;
            std::memcpy(&b, &d, 8);
            std::printf("%x %" PRIx64 "\n", ok ? 1 : 0, b);
        } else if (cmd[0] == 'S') {
            uint64_t hi, lo;
            uint32_t scale;
            if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu32, &hi, &lo, &scale) != 3 || (scale & 255u) > 63u) return 3;
            const U192 v = space_scaled(hi, lo, scale);
            int64_t l[6];
            for (uint32_t i = 0; i < 6u; i++) l[i] = zonal_limb(v, i);
            U192 w;
            const bool ok = zonal_fold(l, w) && w.w0 == v.w0 && w.w1 == v.w1 && w.w2 == v.w2;
            std::printf("%x", ok ? 1 : 0);
            for (int64_t x : l) std::printf(" %" PRIx64, (uint64_t)x);
            std::printf("\n");
        } else if (cmd[0] == 'K') {
            size_t n;
            if (std::fscanf(f, "%zu", &n) != 1) return 3;
            for (size_t i = 0; i < n; i++) {
                uint64_t b, back;
                if (std::fscanf(f, "%" SCNx64, &b) != 1) return 3;
                double d;
                std::memcpy(&d, &b, 8);
                const uint64_t k = zonal_key(d);
                const double u = zonal_unkey(k);
                std::memcpy(&back, &u, 8);
                std::printf("%s%" PRIx64 " %" PRIx64, i ? " " : "", k, back);
            }
            std::printf("\n");
        } else if (cmd[0] == 'R') {
            if (int rc = rank_round(f)) return rc;
        } else if (cmd[0] == 'P') {
            if (int rc = plan(f)) return rc;
        } else {
            return 3;
        }
    }
    std::fclose(f);
    return 0;
}
