// Stand-alone host program over dcdf_amd/csrc/k2r_plan.h (TEST INFRASTRUCTURE ONLY): the plans of the raster's four region calls,
// made on a CPU -- built with -fsanitize=address,undefined by tests/test_raster_plan_host.py.  Reads cases from the file named on
// the command line and prints, for each of the four calls, every list of the plan as the entry point would upload it.
//   case:  T R C tile cs  step(64 | 32)  slab_cap rec_cap wanted  n_bins edge * (n_bins + 1)
//          n_leaves, then per leaf: row0 col0 enc fbits elided bulk_ok
//          nq, then per cube: start end top bottom left right  base_decode base_time sbase_time base_space base_hist moff
//   output: "case", then per call "<call> <code>" ("bounds <code>" first: a batch out of bounds gets no plan), then one line per
//   record: "<list> <field> ..." in the struct's field order, and "stats b w c"; "end" closes the case.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_plan.h"

using namespace k2r;

static void put(const char* tag, std::initializer_list<uint64_t> v) {
    std::printf("%s", tag);
    for (uint64_t x : v) std::printf(" %" PRIu64, x);
    std::printf("\n");
}
static void put_items(const std::vector<WinItem>& items) {
    for (const WinItem& i : items) put("item", {i.chunk, i.inst, i.top, i.bottom, i.left, i.right, i.out_sr, i.out_off});
}
static void put_slabs(const std::vector<Slab>& slabs, uint64_t slab_max, uint32_t fold_nt) {
    for (const Slab& s : slabs) put("slab", {s.item0, s.item1, s.fold0, s.fold1});
    put("slab_max", {slab_max, fold_nt});
}
// the fields every unit type starts with
#define HEAD(u) (uint64_t)(u).chunk, (u).t0, (u).t1, (u).rr, (u).rc, (u).top, (u).bottom, (u).left, (u).right
static void put_fold(const char* tag, const FoldPiece& f) {
    put(tag, {f.nt, f.rows, f.cols, f.sr, f.init, (uint64_t)(int64_t)f.enc, f.fbits, f.elided, f.src, f.o_off, f.s_off, f.psz});
}
static void put_fold(const char* tag, const SpaceFold& f) {
    put(tag, {f.nt, f.rows, f.cols, f.m_sr, (uint64_t)(int64_t)f.enc, f.fbits, f.elided, f.src, f.rec, f.m_off});
}
static void put_fold(const char* tag, const HistFold& f) {
    put(tag, {f.nt, f.rows, f.cols, f.m_sr, (uint64_t)(int64_t)f.enc, f.fbits, f.elided, f.src, f.o_off, f.m_off});
}
template <class Fold>
static void put_walk(const std::vector<Fold>& cfolds, const SlabCutter<Fold>& w) {
    for (const Fold& f : cfolds) put_fold("cfold", f);
    for (const Fold& f : w.folds) put_fold("wfold", f);
    put_items(w.items);
    put_slabs(w.slabs, w.slab_max, w.fold_nt);
}
static void put_stats(const uint64_t s[3]) { put("stats", {s[0], s[1], s[2]}); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    PlanRaster g{};
    uint32_t step, wanted, n_bins;
    uint64_t slab_cap, rec_cap;
    while (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32, &g.T,
                       &g.R, &g.C, &g.tile, &g.cs, &step, &slab_cap, &rec_cap, &wanted, &n_bins) == 10) {
        if (!g.T || !g.R || !g.C || !g.tile || !g.cs || n_bins > HIST_MAX_BINS) return 3;
        g.nti = (g.R + g.tile - 1) / g.tile;
        g.ntj = (g.C + g.tile - 1) / g.tile;
        std::vector<double> edges(n_bins + 1);
        for (double& e : edges)
            if (std::fscanf(f, "%lf", &e) != 1) return 3;
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
        std::vector<uint64_t> bd(nq), bt(nq), st(nq), bs(nq), bh(nq), mo(nq);
        for (size_t q = 0; q < nq; q++) {
            dcdf_cube& c = cubes[q];
            if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64
                            " %" SCNu64, &c.start, &c.end, &c.top, &c.bottom, &c.left, &c.right, &bd[q], &bt[q], &st[q], &bs[q], &bh[q], &mo[q]) != 12)
                return 3;
        }
        const bool node_wise = step == 64;
        std::printf("case\n");
        const int rcb = plan_bounds(g, cubes.data(), nq);
        std::printf("bounds %d\n", rcb);
        if (rcb == DCDF_OK) {
            DecodePlan D;
            std::printf("decode %d\n", plan_decode(g, cubes.data(), nq, bd.data(), node_wise, wanted, D));
            for (const BulkUnit& u : D.units) put("unit", {HEAD(u), u.out_sr, u.out_st, u.out_off});
            put_items(D.items);
            for (const ConstPiece& c : D.consts) put("const", {c.leaf, c.ls, c.le, c.rows, c.cols, c.out_sr, c.out_off, c.out_st});
            put_stats(D.stats);

            TimePlan Tm(slab_cap);
            std::printf("time %d\n", plan_reduce_time(g, cubes.data(), nq, bt.data(), st.data(), node_wise, Tm));
            for (const ReduceUnit& u : Tm.units) put("unit", {HEAD(u), u.sr, u.init, u.o_off, u.s_off, u.psz});
            put_walk(Tm.cfolds, Tm.walk);
            for (const SegRange& r : Tm.ranges) put("range", {r.unit0, r.unit1, r.const0, r.const1, r.slab0, r.slab1});
            for (const MeanPiece& m : Tm.means) put("mean", {m.o_off, m.s_off, m.psz});
            put_stats(Tm.stats);

            SpacePlan S(slab_cap);
            std::printf("space %d\n", plan_reduce_space(g, cubes.data(), nq, bs.data(), mo.data(), node_wise, rec_cap, wanted, S));
            for (const SpaceUnit& u : S.units) put("unit", {HEAD(u), u.m_sr, u.rec, u.m_off});
            put_walk(S.cfolds, S.walk);
            for (const SpaceJob& j : S.jobs) put("job", {j.rec, j.n_slots, j.nt, j.o_off, j.o_stride});
            for (const SpaceBatch& b : S.batches) put("batch", {b.unit0, b.unit1, b.const0, b.const1, b.slab0, b.slab1, b.job0, b.job1, b.job_nt});
            put("rec_max", {S.rec_max});
            put_stats(S.stats);

            HistPlan H(slab_cap);
            std::printf("hist %d\n", plan_histogram(g, cubes.data(), nq, bh.data(), mo.data(), edges.data(), n_bins, node_wise, wanted, H));
            for (const HistUnit& u : H.units) put("unit", {HEAD(u), u.m_sr, u.thr, u.rev, u.o_off, u.m_off});
            put_walk(H.cfolds, H.walk);
            put("thr", {H.thr.size()});
            put_stats(H.stats);
        }
        std::printf("end\n");
    }
    std::fclose(f);
    return 0;
}
