// session_check.cpp -- dcdf_amd/csrc/k2r_session_plan.h without a GPU: reads sessions from a file, prints every list of their
// plans and what the post-run functions decide.  Built by tests/test_session_plan_host.py with ASan + UBSan; test
// infrastructure, not part of libdcdf_k2r.so.
//
//   session_check worst            prints worst_instant_bytes(lg) for lg = 4 .. 8
//   session_check <file>           per session of the file:
//       k out_cap_per_tile cus split(0 default, 1 "0", 2 "all", 3 "tail") max_parts max_wgs(0 = unset) stash_words
//       per_cu[lg = 4..8] (5 numbers)   list_words[lg = 4..8] (5 numbers)      -- stand-ins for k2r_launch.h
//       n, then n lines: instants rows cols dtype stride_t stride_r stride_c base(an address, 0 = null) fractional_bits
//       passes (0 .. 2), then per pass n kernel statuses as a run would leave them on the tiles
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_session_plan.h"

using namespace k2r;

template <class V>
static void line(const char* name, const V& v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
static void lists(const char* name, const std::vector<std::vector<uint32_t>>& vv) {
    std::printf("%s %zu\n", name, vv.size());
    for (const auto& v : vv) line(" ", v);
}
template <class K>
static void tiles_of(const char* name, const std::vector<Group<K>>& groups) {
    std::printf("%s %zu\n", name, groups.size());
    for (const auto& g : groups) line(" ", g.tiles);
}
static void queues(const SessionPlan& p) {
    lists("class_items", p.class_items);
    lists("split", p.split);
    const PartTables t = part_tables(p);
    line("part_first", t.first);
    line("part_items", t.items);
    std::printf("items %zu\n", p.items.size());
    for (const PlanItem& it : p.items)
        std::printf("  %u %u %u %d %" PRIu64 " %" PRIu64 " %d %" PRIu64 "\n", it.tile, it.inst_begin, it.inst_end, (int)it.in_parts_slab,
                    it.out_off, it.out_cap, it.flag, it.shared_off);
}

static bool session(FILE* f) {
    int k, split, per_cu[5];
    unsigned long long out_cap, list_words[5];
    unsigned cus, parts, max_wgs, stash;
    if (std::fscanf(f, "%d %llu %u %d %u %u %u", &k, &out_cap, &cus, &split, &parts, &max_wgs, &stash) != 7) return false;
    for (int& v : per_cu)
        if (std::fscanf(f, "%d", &v) != 1) std::abort();
    for (auto& v : list_words)
        if (std::fscanf(f, "%llu", &v) != 1) std::abort();
    size_t n;
    if (std::fscanf(f, "%zu", &n) != 1) std::abort();
    std::vector<dcdf_tile_desc> tiles(n);
    for (dcdf_tile_desc& t : tiles) {
        unsigned long long base;
        long long st, sr, sc;
        unsigned fbits;
        t = dcdf_tile_desc{};
        if (std::fscanf(f, "%u %u %u %d %lld %lld %lld %llu %u", &t.instants, &t.rows, &t.cols, &t.dtype, &st, &sr, &sc, &base,
                        &fbits) != 9)
            std::abort();
        t.fractional_bits = (decltype(t.fractional_bits))fbits;
        t.stride_t = st; t.stride_r = sr; t.stride_c = sc;
        t.base = (const void*)(uintptr_t)base;  // (never read: the planner looks at its alignment)
    }
    SessionKnobs knobs;
    knobs.split = (SessionKnobs::Split)split;
    knobs.max_parts = parts;
    knobs.max_wgs = max_wgs;
    knobs.stash_words = stash;
    SessionPlan p = plan_session(
        tiles.data(), n, k, (size_t)out_cap, (int)cus, knobs, [&](const EncClass& c) { return per_cu[c.log2s - 4]; },
        [&](const EncClass& c) { return (size_t)list_words[c.log2s - 4]; });

    std::printf("session %zu\n", n);
    line("pre_status", p.pre_status);
    line("tile_class", p.tile_class);
    line("tile_gkey", p.tile_gkey);
    line("minmax_off", p.minmax_off);
    std::printf("classes %zu\n", p.classes.size());
    for (const auto& c : p.classes) std::printf("  %d %d %d\n", c.key.log2s, (int)c.key.padded, c.key.vec);
    tiles_of("class_tiles", p.classes);
    std::printf("generic_keys");
    for (const auto& g : p.generic_groups) std::printf(" %u", g.key);
    std::printf("\n");
    tiles_of("generic_tiles", p.generic_groups);
    line("grid", p.grid);
    line("order_off", p.order_off);
    line("lists_off", p.lists_off);
    std::printf("totals %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %zu %zu %zu\n", p.out_total, p.parts_total, p.shared_total,
                p.minmax_total, p.flags, p.order_total, p.lists_total);
    queues(p);

    int passes;
    if (std::fscanf(f, "%d", &passes) != 1) std::abort();
    std::printf("n_passes %d\n", passes);
    std::vector<TileResult> res(p.items.size());
    for (int pass = 0; pass < passes; pass++) {
        std::printf("pass %d\n", pass);
        for (size_t i = 0; i < n; i++)
            if (std::fscanf(f, "%d", &res[i].status) != 1) std::abort();
        if (pass == 0) {  // (dcdf_encoder_run: the splice lists are those of the run itself, before any retry)
            const PartTables s = splice_tables(p, res.data());
            line("splice_first", s.first);
            line("splice_items", s.items);
        }
        const Retry r = plan_retry(p, tiles.data(), res.data());
        lists("again", r.again);
        line("retry_tiles", r.tiles);
        line("retry_own_cap", r.own_cap);
        std::printf("unsplit %d\n", (int)r.unsplit);
        if (r.unsplit) drop_parts(p);
        queues(p);
        const auto declined = declined_groups(p, res.data());
        std::printf("declined_keys");
        for (const auto& g : declined) std::printf(" %u", g.key);
        std::printf("\n");
        tiles_of("declined_tiles", declined);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (std::string_view(argv[1]) == "worst") {
        for (uint32_t lg = 4; lg <= 8; lg++) std::printf("%" PRIu64 "\n", worst_instant_bytes(lg));
        return 0;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    while (session(f)) {}
    std::fclose(f);
    return 0;
}
