// k2r_session_plan.h -- the host plan of an encode session (dcdf_encoder_create / dcdf_encoder_run), as plain C++.
//
// Which kernel encodes a tile, which tiles are encoded in speculative parts and where these are cut, the order of every class's
// work queue, where every item's output slot lies, and after a run which tiles run again and how.  No HIP and no getenv: the
// session (k2r_session.hip) reads the knobs, allocates, turns offsets into pointers and launches; tests/sim/session_check.cpp
// compiles this header with g++ and prints every list.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/dcdf_k2r.h"
#include "k2r_common.h"
#include "k2r_ref_tree.h"

namespace k2r {

// The environment of one dcdf_encoder_create (read there, once per session).
struct SessionKnobs {
    enum Split { kSplitDefault, kSplitOff, kSplitAll, kSplitTail };
    Split split = kSplitDefault;  // K2R_SPLIT: unset / "0" / "all" / "tail"
    uint32_t max_parts = 8;       // K2R_PARTS, 2..8 (8 parts: 0.934 of linear on the N = 8 share, 4: 0.919; profiles/r04r)
    uint32_t max_wgs = 0;         // K2R_MAX_WGS (diagnostics), at least 1; 0 = unset
    uint32_t stash_words = 0;     // K2R_STASH_WORDS (A/B runs): caps the LDS words of the log stash; 1 = always re-read
};

inline size_t elem_size(int dtype) { return (dtype == DCDF_I32 || dtype == DCDF_F32) ? 4 : 8; }

inline uint32_t sidelen_log2(uint32_t rows, uint32_t cols) {  // snapshot.rs:118-119 for k = 2
    uint32_t m = std::max(rows, cols);
    uint32_t lg = 0;
    while ((1u << lg) < m) lg++;
    return lg;
}

// a tile somebody can read: a base, no empty dimension, one of the four types
inline bool desc_ok(const dcdf_tile_desc& t) {
    if (!t.base || t.instants == 0 || t.rows == 0 || t.cols == 0) return false;
    return t.dtype == DCDF_I32 || t.dtype == DCDF_I64 || t.dtype == DCDF_F32 || t.dtype == DCDF_F64;
}

constexpr uint64_t kGenericMaxSidelen = 1024;  // universal kernel: level arrays in HBM scratch, ~77 B per node

// returns DCDF_OK and either a fused-kernel class (*generic_key == 0) or the universal kernel's key (k << 8 | H)
inline int validate_tile(const dcdf_tile_desc& t, int k, EncClass* cls, uint32_t* generic_key) {
    *generic_key = 0;
    if (!desc_ok(t)) return DCDF_ERR_BAD_ARG;
    if ((t.dtype == DCDF_F32 || t.dtype == DCDF_F64) && t.fractional_bits > 62) return DCDF_ERR_BAD_ARG;
    if (k < 2 || k > 16) return DCDF_ERR_BAD_ARG;
    const uint32_t lg = sidelen_log2(t.rows, t.cols);
    if (k != 2 || lg < 4 || lg > 8) {  // outside the fused kernel (k = 2, sidelen 16 .. 256): any k, sidelen 1 .. 1024
        // depth and sidelen of the tile's tree, by the reference's own f64 formula (k2r_ref_tree.h)
        const uint64_t m = std::max(t.rows, t.cols);
        if (ref_sidelen(m, (uint32_t)k) > kGenericMaxSidelen) return DCDF_ERR_UNSUPPORTED;
        *generic_key = ((uint32_t)k << 8) | ref_levels(m, (uint32_t)k);
        return DCDF_OK;
    }
    const uint32_t S = 1u << lg;
    cls->log2s = (int)lg;
    cls->padded = t.rows != S || t.cols != S;
    // 16-byte row loads: unit column stride, rows and instants 16-byte aligned, 32-bit byte offsets inside an instant
    const uint64_t esz = elem_size(t.dtype);
    const int64_t al = (int64_t)(16 / esz);
    const bool rows16 = !cls->padded && t.stride_c == 1 && (t.stride_r % al) == 0 && t.stride_r > 0 && (t.stride_t % al) == 0 &&
                        ((uintptr_t)t.base % 16) == 0 &&
                        ((uint64_t)(t.rows - 1) * (uint64_t)t.stride_r + t.cols) * esz < (1ull << 31);
    cls->vec = !rows16 ? 0 : (t.dtype == DCDF_I32 ? 1 : (t.dtype == DCDF_F32 ? 2 : (t.dtype == DCDF_I64 ? 3 : 4)));
    return DCDF_OK;
}

// ---- speculative parts: which tiles of a class to encode as several work items ---------------------------------------------
// A chunk is the unit of work (its instants are sequential) and a workgroup owns a CU, so when a GPU holds only a few
// chunks per CU the end of the work queue leaves CUs idle: 384 chunks on 256 CUs take two chunk-times, not 1.5, and whatever
// the count, the last chunk popped runs a whole chunk-time after the queue is empty.  Encoding the chunks at the END of the
// (longest-first) queue in parts of decreasing length (T/2, T/4, T/8, T/8: guided self-scheduling) fills that tail with
// small items.  A part costs its instants plus a little (the wait for the first part's snapshot copy, the splice), and a
// failed speculation costs a whole re-encode, so only tiles of the last rounds are split, and only when the queue is short:
// n <= 4 * wgs.  K2R_SPLIT=0 disables, =all forces every tile (tests), =tail forces the last two rounds whatever n.
// `inst`: the instants of the class's tiles, longest first.  Returns how many tiles at the END of it are split: the candidate
// tail -- or none at all as soon as ONE tile of it has fewer than 4 instants (longest first, the short ones are the tail's last,
// where the shrinking loop does not look).  One 3-instant tile therefore keeps every tile of its class whole under "all":
// today's rule, pinned by tests/test_session_plan_host.py, and the reason tests keep short tiles out of a split session.
inline size_t plan_split(const std::vector<uint32_t>& inst, uint32_t wgs, SessionKnobs::Split mode) {
    const size_t n = inst.size();
    auto splittable = [&](size_t ns) {  // the last ns tiles, shrunk to those with at least 4 instants
        while (ns > 0 && inst[n - ns] < 4) ns--;
        size_t ok = 0;
        for (size_t q = n - ns; q < n; q++) ok += inst[q] >= 4;
        return ok == ns ? ns : (size_t)0;
    };
    if (mode == SessionKnobs::kSplitOff) return 0;
    if (mode == SessionKnobs::kSplitAll) return splittable(n);
    const size_t tail = std::min<size_t>(n, 2 * (size_t)wgs);
    if (mode == SessionKnobs::kSplitTail) return splittable(tail);
    if (n > 4 * (size_t)wgs) return 0;
    return splittable(tail);
}
// the instants at which the parts of a T-instant tile begin (after 0): T/2, then half of what is left, ... (<= max_parts parts)
inline std::vector<uint32_t> part_bounds(uint32_t T, uint32_t max_parts) {
    std::vector<uint32_t> b;
    uint32_t at = 0, left = T;
    while (b.size() + 2 <= max_parts && left >= 4) {
        at += (left + 1) / 2;
        left -= (left + 1) / 2;
        b.push_back(at);
    }
    return b;
}

// Upper bound of one serialized instant (all values 4 bytes): used when the default slot overflows.
inline uint64_t worst_instant_bytes(uint32_t lg) {
    const uint64_t maxv = ((1ull << (2 * (lg + 1))) - 1) / 3, maxt = ((1ull << (2 * lg)) - 1) / 3;
    auto bm = [](uint64_t n) { return 8 + 4 * (n / 128) + 4 * ((n + 31) / 32); };
    return 13 + 2 * bm(maxt) + (1 + 4 * (bm(maxv) + maxv)) + (1 + 4 * (bm(maxt) + maxt));
}

// tiles that share a key, in the order the keys first occur
template <class K>
struct Group {
    K key;
    std::vector<uint32_t> tiles;
};
template <class K>
size_t group_of(std::vector<Group<K>>& groups, const K& key) {
    size_t g = 0;
    for (; g < groups.size(); g++)
        if (groups[g].key == key) return g;
    groups.push_back(Group<K>{key, {}});
    return g;
}

// One work item = one TileArgs record: items [0, n) are the tiles, the rest the continuations of split tiles.
struct PlanItem {
    uint32_t tile = 0;                      // whose instants
    uint32_t inst_begin = 0, inst_end = 0;  // TileArgs: [inst_begin, inst_end), inst_end == 0 = the whole tile
    bool in_parts_slab = false;             // out_off counts from the main slab (a tile's own slot) or from the parts' slab
    uint64_t out_off = 0, out_cap = 0;
    int32_t flag = -1;                      // split tiles and their parts: the 16-byte flag record, and ...
    uint64_t shared_off = 0;                // ... where the shared compact copy of instant 0 starts
};

struct SessionPlan {
    size_t n = 0;                     // tiles
    std::vector<int32_t> pre_status;  // validate_tile per tile
    std::vector<Group<EncClass>> classes;          // the fused kernel's tiles, longest first inside a class
    std::vector<Group<uint32_t>> generic_groups;   // the universal kernel's (k2r_generic.hip): key = k << 8 | H
    std::vector<int32_t> tile_class;  // per tile: its index into `classes`, or -1 and ...
    std::vector<uint32_t> tile_gkey;  // ... the universal kernel's key (0 for a tile of a class)
    std::vector<uint64_t> minmax_off;
    std::vector<PlanItem> items;
    std::vector<std::vector<uint32_t>> class_items;  // per class: the launch order (tile indices and extra indices >= n)
    std::vector<std::vector<uint32_t>> split;        // per split tile: {tile, continuation items in order}
    std::vector<uint32_t> grid;                      // per class: workgroups
    std::vector<size_t> order_off, lists_off;        // per class: offset into the order lists (u32) and the scratch lists (u64)
    uint64_t out_total = 0, parts_total = 0, shared_total = 0, minmax_total = 0;  // bytes, bytes, bytes, int64 words
    size_t flags = 0;                                // flag records (the split tiles at creation)
    size_t order_total = 0, lists_total = 0;
};

// per_cu(cls) = encode_blocks_per_cu, list_words(cls) = encode_list_words (k2r_launch.h)
template <class PerCu, class ListWords>
SessionPlan plan_session(const dcdf_tile_desc* tiles, size_t n, int k, size_t out_cap_per_tile, int cus, const SessionKnobs& knobs,
                         PerCu&& per_cu, ListWords&& list_words) {
    SessionPlan p;
    p.n = n;
    p.pre_status.resize(n);
    p.tile_class.assign(n, -1);
    p.tile_gkey.assign(n, 0);
    p.minmax_off.resize(n);
    p.items.reserve(n + n / 2);
    p.items.resize(n);
    for (size_t i = 0; i < n; i++) {
        const dcdf_tile_desc& t = tiles[i];
        EncClass cls{};
        uint32_t gkey = 0;
        const int st = validate_tile(t, k, &cls, &gkey);
        p.pre_status[i] = st;
        p.items[i].tile = (uint32_t)i;
        if (st != DCDF_OK) continue;
        if (gkey) {
            p.tile_gkey[i] = gkey;
            p.generic_groups[group_of(p.generic_groups, gkey)].tiles.push_back((uint32_t)i);
        } else {
            const size_t ci = group_of(p.classes, cls);
            p.classes[ci].tiles.push_back((uint32_t)i);
            p.tile_class[i] = (int32_t)ci;
        }
        uint64_t cap = out_cap_per_tile ? out_cap_per_tile : (uint64_t)t.instants * t.rows * t.cols * 4 + 4096;
        cap = (cap + 255) & ~255ull;
        p.items[i].out_off = p.out_total;
        p.items[i].out_cap = cap;
        p.out_total += cap;
        p.minmax_off[i] = p.minmax_total;
        p.minmax_total += 2ull * t.instants;
    }
    // per-class launch geometry; which tiles are encoded in speculative parts (plan_split)
    p.class_items.resize(p.classes.size());
    for (size_t ci = 0; ci < p.classes.size(); ci++) {
        const EncClass& c = p.classes[ci].key;
        auto& v = p.classes[ci].tiles;
        // longest chunks first: the tail of the work queue is then made of the short ones
        std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return tiles[a].instants > tiles[b].instants; });
        uint32_t wgs = (uint32_t)((uint64_t)cus * (uint64_t)per_cu(c));
        if (knobs.max_wgs) wgs = std::min(wgs, knobs.max_wgs);
        std::vector<uint32_t> inst(v.size());
        for (size_t q = 0; q < v.size(); q++) inst[q] = tiles[v[q]].instants;
        const size_t ns = plan_split(inst, std::max(1u, wgs), knobs.split);  // the LAST ns tiles of v are split
        struct Queued { uint32_t idx, cost, cont; };
        std::vector<Queued> queue;
        queue.reserve(v.size() + ns * knobs.max_parts);
        const uint64_t cmp_bytes = ((2ull << (2 * c.log2s)) + 255) & ~255ull;  // 2 bytes per cell of the padded tile
        for (size_t q = 0; q < v.size(); q++) {
            const uint32_t ti = v[q], T = tiles[ti].instants;
            if (q + ns < v.size()) {
                queue.push_back({ti, T, 0});
                continue;
            }
            const std::vector<uint32_t> at = part_bounds(T, knobs.max_parts);
            std::vector<uint32_t> parts{ti};
            p.items[ti].inst_end = at[0];
            p.items[ti].flag = (int32_t)p.split.size();
            p.items[ti].shared_off = p.shared_total;
            p.shared_total += cmp_bytes;
            queue.push_back({ti, at[0], 0});
            uint32_t prev_cost = at[0];
            for (size_t q2 = 0; q2 < at.size(); q2++) {
                const uint32_t m0 = at[q2], m1 = q2 + 1 < at.size() ? at[q2 + 1] : T, bi = (uint32_t)p.items.size();
                PlanItem b = p.items[ti];
                b.inst_begin = m0;
                b.inst_end = m1;
                b.out_cap = ((p.items[ti].out_cap * (m1 - m0) + T - 1) / T + 4096 + 255) & ~255ull;
                b.in_parts_slab = true;
                b.out_off = p.parts_total;
                p.parts_total += b.out_cap;
                p.items.push_back(b);
                parts.push_back(bi);
                prev_cost = std::min(prev_cost, m1 - m0);  // (never sorted before the part it follows)
                queue.push_back({bi, prev_cost, 1});
            }
            p.split.push_back(std::move(parts));
        }
        // longest first; at equal length a first part before any continuation -- with first parts at least as long as their
        // continuations, every continuation is popped after the part it waits for (k2r_encode.h)
        std::stable_sort(queue.begin(), queue.end(),
                         [](const Queued& a, const Queued& b) { return a.cost != b.cost ? a.cost > b.cost : a.cont < b.cont; });
        p.class_items[ci].reserve(queue.size());
        for (const Queued& it : queue) p.class_items[ci].push_back(it.idx);
        p.grid.push_back(std::max(1u, (uint32_t)std::min<uint64_t>(queue.size(), wgs)));
        p.order_off.push_back(p.order_total);
        p.order_total += queue.size();
        p.lists_off.push_back(p.lists_total);
        p.lists_total += (size_t)p.grid.back() * list_words(c);
    }
    p.flags = p.split.size();
    return p;
}

// `groups` as k_stitch reads them: items = the groups one after the other, first[j] .. first[j + 1] = group j
struct PartTables {
    std::vector<uint32_t> first{0}, items;
};
template <class Keep>
PartTables part_tables(const std::vector<std::vector<uint32_t>>& groups, Keep&& keep) {
    PartTables t;
    for (const auto& parts : groups)
        if (keep(parts)) {
            t.items.insert(t.items.end(), parts.begin(), parts.end());
            t.first.push_back((uint32_t)t.items.size());
        }
    return t;
}
inline PartTables part_tables(const SessionPlan& p) {
    return part_tables(p.split, [](const std::vector<uint32_t>&) { return true; });
}
// the split tiles whose parts checked out in a run (k_stitch<false> left ST_OK): only those are appended by materialize() -- a
// tile that is re-encoded whole afterwards (retry, universal kernel) has all its bytes already
inline PartTables splice_tables(const SessionPlan& p, const TileResult* res) {
    return part_tables(p.split, [&](const std::vector<uint32_t>& parts) { return res[parts[0]].status == ST_OK; });
}

// ---- after a run ------------------------------------------------------------------------------------------------------------
// Tiles whose slot was too small (ST_OUT_CAPACITY) are encoded again, alone, into a worst-case slot of their own; tiles whose
// speculative parts did not splice (ST_RESPLIT) are encoded again whole -- which may then turn out too big for the slot: the
// caller asks a second time.  Either way the tile is whole from now on: a block boundary in its first half, or a slot too
// small, would come back on every run.
struct Retry {
    std::vector<std::vector<uint32_t>> again;  // per class: the tiles to run
    std::vector<uint32_t> tiles;               // all of them: each has become whole in the plan (inst_end 0, no flag)
    std::vector<uint64_t> own_cap;             // per entry of `tiles`: 0 = it keeps its slot, else the bytes of the new one
    bool unsplit = false;                      // one of them had been split: drop_parts() after the run
};
inline Retry plan_retry(SessionPlan& p, const dcdf_tile_desc* tiles, const TileResult* res) {
    Retry r;
    r.again.resize(p.classes.size());
    for (size_t ci = 0; ci < p.classes.size(); ci++)
        for (uint32_t ti : p.classes[ci].tiles) {
            const int32_t st = res[ti].status;
            if (st != ST_OUT_CAPACITY && st != ST_RESPLIT) continue;
            const uint64_t worst = 6 + (uint64_t)tiles[ti].instants * (1 + worst_instant_bytes((uint32_t)p.classes[ci].key.log2s));
            r.unsplit = r.unsplit || p.items[ti].inst_end != 0;
            p.items[ti].inst_end = 0;
            p.items[ti].flag = -1;
            r.again[ci].push_back(ti);
            r.tiles.push_back(ti);
            r.own_cap.push_back(st == ST_OUT_CAPACITY ? worst : 0);
        }
    return r;
}
// drops the parts (extra items) of the tiles that are whole from now on, from `split` and from every class's queue
inline void drop_parts(SessionPlan& p) {
    std::vector<uint8_t> gone(p.items.size(), 0);
    std::vector<std::vector<uint32_t>> keep_split;
    for (auto& parts : p.split) {
        if (p.items[parts[0]].inst_end == 0) {
            for (size_t q = 1; q < parts.size(); q++) gone[parts[q]] = 1;
            continue;
        }
        keep_split.push_back(std::move(parts));
    }
    p.split.swap(keep_split);
    for (auto& items : p.class_items)
        items.erase(std::remove_if(items.begin(), items.end(), [&](uint32_t it) { return gone[it] != 0; }), items.end());
}
// the tiles the fused kernel declined at run time (a stored value beyond its 2^30 contract: ST_UNSUPPORTED), grouped for the
// universal kernel
inline std::vector<Group<uint32_t>> declined_groups(const SessionPlan& p, const TileResult* res) {
    std::vector<Group<uint32_t>> declined;
    for (const auto& c : p.classes)
        for (uint32_t ti : c.tiles)
            if (res[ti].status == ST_UNSUPPORTED) declined[group_of(declined, (2u << 8) | (uint32_t)c.key.log2s)].tiles.push_back(ti);
    return declined;
}

}  // namespace k2r
