// Stand-alone host program over dcdf_amd/csrc/k2r_spell.h and plan_spells of k2r_plan.h (TEST INFRASTRUCTURE ONLY), built with
// -fsanitize=address,undefined by tests/test_spells_host.py.  Three checks, each printing "ok <name> <count>":
//   (a) cuts   every hit series of length <= 12 folded in one go equals the same series folded through stored and re-loaded state
//              planes (spell_plane) at every single cut and every pair of cuts, and equals a plain scan of the series;
//   (b) hits   the int32 and int64 hit tests agree with value_bounds' set, and with the decoded value itself, for all four
//              encodings, fractional bits 0, 3 and 62, at and next to every end of ranges that are empty, empty only after clamping,
//              that contain the hole, that are unbounded on either side;
//   (c) plan   plan_spells on the geometries of tests/test_raster_plan_host.py: every cell of every cube is covered at each of its
//              instants exactly once and in instant order, segments ascend, init is set exactly where dt == 0, dt is the piece's
//              first instant less the cube's, the range is value_bounds' for the leaf.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_plan.h"

using namespace k2r;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static bool same(const SpellState& a, const SpellState& b, bool with_cur) {
    return a.count == b.count && a.longest == b.longest && a.lstart == b.lstart && a.first == b.first && a.last == b.last && (!with_cur || a.cur == b.cur);
}

// ---- (a) ---------------------------------------------------------------------------------------------------------------------
// the five numbers by a plain scan of the runs, written apart from spell_step
static SpellState scan(uint32_t bits, uint32_t len) {
    SpellState s{0, 0, 0, SPELL_NONE, SPELL_NONE, SPELL_NONE};
    uint32_t i = 0;
    while (i < len) {
        if (!((bits >> i) & 1u)) {
            i++;
            continue;
        }
        uint32_t j = i;
        while (j < len && ((bits >> j) & 1u)) j++;
        s.count += j - i;
        if (j - i > s.longest) {
            s.longest = j - i;
            s.lstart = i;
        }
        if (s.first == SPELL_NONE) s.first = i;
        s.last = j - 1;
        i = j;
    }
    return s;
}
// the instants [a, b) of one cell through its planes: load unless init, step, store -- what a piece of the plan does
static void piece(uint32_t bits, uint32_t a, uint32_t b, bool init, uint32_t ops, uint32_t* dst, uint32_t* scr, uint64_t o_off, uint64_t s_off,
                  uint64_t psz) {
    const uint32_t live = spell_live(ops);
    uint32_t* const pl[6] = {spell_plane(SP_COUNT, dst, scr, ops, o_off, s_off, psz),  spell_plane(SP_LONGEST, dst, scr, ops, o_off, s_off, psz),
                             spell_plane(SP_LSTART, dst, scr, ops, o_off, s_off, psz), spell_plane(SP_FIRST, dst, scr, ops, o_off, s_off, psz),
                             spell_plane(SP_LAST, dst, scr, ops, o_off, s_off, psz),   spell_plane(SP_CUR, dst, scr, ops, o_off, s_off, psz)};
    SpellState s = spell_init();
    if (!init) {
        if (live & SP_COUNT) s.count = *pl[0];
        if (live & SP_LONGEST) s.longest = *pl[1];
        if (live & SP_LSTART) s.lstart = *pl[2];
        if (live & SP_FIRST) s.first = *pl[3];
        if (live & SP_LAST) s.last = *pl[4];
        if (live & SP_CUR) s.cur = *pl[5];
    }
    for (uint32_t i = a; i < b; i++) spell_step(s, i, ((bits >> i) & 1u) != 0);
    if (live & SP_COUNT) *pl[0] = s.count;
    if (live & SP_LONGEST) *pl[1] = s.longest;
    if (live & SP_LSTART) *pl[2] = s.lstart;
    if (live & SP_FIRST) *pl[3] = s.first;
    if (live & SP_LAST) *pl[4] = s.last;
    if (live & SP_CUR) *pl[5] = s.cur;
}
static uint64_t check_cuts() {
    uint64_t n = 0;
    constexpr uint64_t PSZ = 3, CELL = 1;  // planes of three cells, the middle one used: its neighbours must stay untouched
    constexpr uint32_t SENT = 0xabcd1234u;
    const uint32_t op_sets[] = {SP_ALL, SP_LSTART, SP_COUNT, SP_LONGEST, SP_FIRST | SP_LAST, SP_LSTART | SP_LAST};
    for (uint32_t len = 0; len <= 12; len++)
        for (uint32_t bits = 0; bits < (1u << len); bits++) {
            SpellState whole = spell_init();
            for (uint32_t i = 0; i < len; i++) spell_step(whole, i, ((bits >> i) & 1u) != 0);
            CHECK(same(whole, scan(bits, len), false));
            for (uint32_t ops : op_sets) {
                if (ops != SP_ALL && (bits % 7u) != 0) continue;  // (the other op sets on a seventh of the series)
                const uint32_t n_out = popc32(ops), n_scr = popc32(spell_live(ops) & ~ops);
                for (uint32_t c1 = 0; c1 <= len; c1++)
                    for (uint32_t c2 = c1; c2 <= len; c2++) {
                        std::vector<uint32_t> dst(n_out * PSZ, SENT), scr(n_scr * PSZ + 1, SENT);
                        piece(bits, 0, c1, true, ops, dst.data(), scr.data(), CELL, CELL, PSZ);
                        piece(bits, c1, c2, false, ops, dst.data(), scr.data(), CELL, CELL, PSZ);
                        piece(bits, c2, len, false, ops, dst.data(), scr.data(), CELL, CELL, PSZ);
                        uint32_t at = 0;
                        const uint32_t want[5] = {whole.count, whole.longest, whole.lstart, whole.first, whole.last};
                        for (uint32_t b = 0; b < 5; b++)
                            if (ops & (1u << b)) {
                                CHECK(dst[at * PSZ + CELL] == want[b]);
                                CHECK(dst[at * PSZ] == SENT && dst[at * PSZ + 2] == SENT);
                                at++;
                            }
                        for (uint32_t p = 0; p < n_scr; p++) CHECK(scr[p * PSZ] == SENT && scr[p * PSZ + 2] == SENT);
                        CHECK(scr[n_scr * PSZ] == SENT);
                        n++;
                    }
            }
        }
    return n;
}

// ---- (b) ---------------------------------------------------------------------------------------------------------------------
static bool decoded_hit(int32_t enc, uint32_t fbits, int64_t n, double lower, double upper) {
    if (lower > upper) std::swap(lower, upper);
    if (enc == ENC_I32 || enc == ENC_I64) return (double)n >= std::ceil(lower) && (double)n <= std::floor(upper);  // (|n| <= 2^31 here: exact)
    if (n == 0) return false;
    const double v = enc == ENC_F32 ? (double)from_fixed_f32(n, fbits) : from_fixed_f64(n, fbits);
    return lower <= v && v <= upper;
}
static uint64_t check_hits() {
    uint64_t n_checked = 0;
    const double inf = __builtin_inf();
    const int32_t encs[4] = {ENC_I32, ENC_I64, ENC_F32, ENC_F64};
    const uint32_t fbs[3] = {0, 3, 62};
    for (int32_t enc : encs)
        for (uint32_t fb : fbs) {
            const bool is_float = enc == ENC_F32 || enc == ENC_F64;
            // one stored step in value units, and a scale that keeps the narrow integers inside the ranges' reach
            const double unit = !is_float ? 1.0 : fb == 62 ? 1.0 / 9223372036854775808.0 : 1.0 / (double)((int64_t)1 << (fb + 1));
            std::vector<std::pair<double, double>> ranges = {
                {0.5 * unit, 0.5 * unit},                  // between two values: empty
                {0.25 * unit, 0.75 * unit},                // the same, two-sided
                {1099511627776.0 * unit * 4, inf},         // beyond int32 in stored integers: empty only after clamping
                {-inf, -1099511627776.0 * unit * 4},       //
                {1099511627776.0 * unit * 4, 1099511627777.0 * unit * 8},
                {-3.0 * unit, 5.0 * unit},                 // around zero: the hole of a float leaf
                {-1000.0 * unit, 1000.0 * unit},
                {5.0 * unit, -3.0 * unit},                 // reversed
                {-inf, 7.0 * unit},                        // unbounded on either side, and on both
                {-7.0 * unit, inf},
                {-inf, inf},
                {-inf, -inf},
                {inf, inf},
                {0.0, 0.0},
                {-2147483648.0 * unit, 2147483647.0 * unit},
                {-2147483649.0 * unit, 2147483648.0 * unit},
                {1073741823.0 * unit, 1073741824.0 * unit},
                {123.0 * unit, 123.0 * unit},
            };
            for (const auto& r : ranges) {
                ValueRange vr;
                CHECK(value_bounds(enc, fb, r.first, r.second, &vr));
                const SpellRange32 r32 = spell_range32(vr);
                const SpellRange64 r64 = spell_range64(vr);
                CHECK(vr.empty == ((r64.flags & SH_EMPTY) != 0));
                if (r32.flags & SH_EMPTY) CHECK(vr.empty || vr.lo > INT32_MAX || vr.hi < INT32_MIN);
                std::vector<int64_t> ns = {-2, -1, 0, 1, 2, INT32_MIN, (int64_t)INT32_MIN + 1, INT32_MAX, (int64_t)INT32_MAX - 1, -(1 << 30), (1 << 30) - 1,
                                           1 << 30, (int64_t)INT32_MIN - 1, (int64_t)INT32_MAX + 1, INT64_MIN, INT64_MAX};
                for (int64_t end : {vr.lo, vr.hi, (int64_t)r32.lo, (int64_t)r32.hi, r64.lo, r64.hi})
                    for (int64_t d = -2; d <= 2; d++) {
                        if ((d < 0 && end < INT64_MIN - d) || (d > 0 && end > INT64_MAX - d)) continue;
                        ns.push_back(end + d);
                    }
                for (int64_t n : ns) {
                    const bool want = !vr.empty && vr.lo <= n && n <= vr.hi && !(vr.hole && n == 0);
                    CHECK(spell_hit64(n, r64.lo, r64.hi, r64.flags) == want);
                    if (n >= INT32_MIN && n <= INT32_MAX) {
                        CHECK(spell_hit32((int32_t)n, r32.lo, r32.hi, r32.flags) == want);
                        // the set is the decoded value's own: checked where the decoder's arithmetic is exact and defined
                        if (n > INT32_MIN) CHECK(decoded_hit(enc, fb, n, r.first, r.second) == want);
                    }
                    n_checked++;
                }
            }
        }
    // what the issue warns of: the unsigned one-compare form accepts every n for lo = 1, hi = 0; the explicit flag does not
    ValueRange e;
    CHECK(value_bounds(ENC_I32, 0, 0.5, 0.5, &e) && e.empty);
    for (int32_t n : {INT32_MIN, -1, 0, 1, 2, INT32_MAX}) CHECK(!spell_hit32(n, spell_range32(e).lo, spell_range32(e).hi, spell_range32(e).flags));
    return n_checked;
}

// ---- (c) ---------------------------------------------------------------------------------------------------------------------
struct Geo {
    PlanRaster g;
    std::vector<PlanLeaf> leaves;
};
static Geo plain(int table) {  // 0: all bulk, 1: all walk, 2: checker
    Geo G;
    G.g = PlanRaster{20, 100, 200, 96, 9, 2, 3, nullptr};
    for (uint32_t leaf = 0; leaf < 18; leaf++) {
        const uint32_t seg = leaf / 6, ti = leaf / 3 % 2, tj = leaf % 3;
        G.leaves.push_back(PlanLeaf{0, 0, ENC_I32, 0, 0, (uint8_t)(table == 0 ? 1 : table == 1 ? 0 : (seg + ti + tj) % 2)});
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
static uint64_t check_plan_case(Geo& G, const std::vector<dcdf_cube>& cubes, const std::vector<double>& lower, const std::vector<double>& upper,
                                bool node_wise, uint64_t slab_cap) {
    G.g.leaves = G.leaves.data();
    const PlanRaster& g = G.g;
    const size_t nq = cubes.size();
    std::vector<uint64_t> base(nq), sbase(nq), plane(nq);
    std::vector<dcdf_cube> nc(nq);
    uint64_t at = 0, sat = 0, want_stats[3] = {0, 0, 0};
    for (size_t q = 0; q < nq; q++) {
        nc[q] = norm_cube(cubes[q]);
        plane[q] = cube_cells(nc[q]) ? (uint64_t)(nc[q].bottom - nc[q].top) * (nc[q].right - nc[q].left) : 0;
        base[q] = at + 5;
        sbase[q] = sat + 2;
        at = base[q] + plane[q];
        sat = sbase[q] + plane[q];
    }
    CHECK(plan_bounds(g, cubes.data(), nq) == DCDF_OK);
    SpellPlan P(slab_cap);
    CHECK(plan_spells(g, cubes.data(), lower.data(), upper.data(), nq, base.data(), sbase.data(), node_wise, P) == DCDF_OK);
    // next[q][cell]: the instant (from the cube's first) the cell's next record must start at
    std::vector<std::vector<uint32_t>> next(nq);
    for (size_t q = 0; q < nq; q++) next[q].assign(plane[q], 0);
    auto cube_of = [&](uint64_t o_off) {
        for (size_t q = 0; q < nq; q++)
            if (plane[q] && o_off >= base[q] && o_off < base[q] + plane[q]) return q;
        CHECK(!"an offset in no cube");
        return (size_t)0;
    };
    // a record: leaf, its first instant in the segment, nt, the rectangle's first raster cell (or -1: elided, any cell of the leaf)
    auto paint = [&](uint32_t leaf, uint32_t inst, uint32_t nt, int64_t r0, int64_t c0, uint32_t rows, uint32_t cols, uint32_t sr, uint32_t init,
                     uint32_t dt, uint64_t o_off, uint64_t s_off, uint64_t psz, int64_t lo, int64_t hi, uint32_t flags, bool narrow) {
        const size_t q = cube_of(o_off);
        const dcdf_cube& c = nc[q];
        const uint32_t wc = c.right - c.left, seg = leaf / (g.nti * g.ntj), ti = leaf / g.ntj % g.nti, tj = leaf % g.ntj;
        CHECK(sr == wc && psz == plane[q] && s_off - sbase[q] == o_off - base[q]);
        CHECK(nt > 0 && inst + nt <= g.cs && seg * g.cs + inst >= c.start && seg * g.cs + inst + nt <= c.end);
        CHECK(dt == seg * g.cs + inst - c.start);
        CHECK((init != 0) == (dt == 0));
        const uint64_t p = o_off - base[q];
        const uint32_t pr = (uint32_t)(p / wc), pc = (uint32_t)(p % wc);
        CHECK(pc + cols <= wc && pr + rows <= c.bottom - c.top && rows > 0 && cols > 0);
        if (r0 >= 0) CHECK(r0 == (int64_t)c.top + pr && c0 == (int64_t)c.left + pc);
        CHECK((c.top + pr) / g.tile == ti && (c.top + pr + rows - 1) / g.tile == ti && (c.left + pc) / g.tile == tj && (c.left + pc + cols - 1) / g.tile == tj);
        for (uint32_t r = 0; r < rows; r++)
            for (uint32_t cc = 0; cc < cols; cc++) {
                uint32_t& nx = next[q][(uint64_t)(pr + r) * wc + pc + cc];
                CHECK(nx == dt);  // exactly once, in instant order
                nx = dt + nt;
            }
        ValueRange vr;
        CHECK(value_bounds(g.leaves[leaf].enc, g.leaves[leaf].fbits, lower[q], upper[q], &vr));
        if (narrow) {
            const SpellRange32 w = spell_range32(vr);
            CHECK(lo == w.lo && hi == w.hi && flags == w.flags);
        } else {
            const SpellRange64 w = spell_range64(vr);
            CHECK(lo == w.lo && hi == w.hi && flags == w.flags);
        }
        return seg;
    };
    uint64_t records = 0;
    int64_t prev_seg = -1;
    size_t a_unit = 0, a_const = 0, a_slab = 0;
    for (const SegRange& R : P.ranges) {
        CHECK(R.unit0 == a_unit && R.const0 == a_const && R.slab0 == a_slab);
        CHECK(R.unit1 > R.unit0 || R.const1 > R.const0 || R.slab1 > R.slab0);
        a_unit = R.unit1, a_const = R.const1, a_slab = R.slab1;
        int64_t seg_of = -1;
        auto in_seg = [&](uint32_t seg) {
            CHECK(seg_of < 0 || seg_of == (int64_t)seg);
            seg_of = seg;
            records++;
        };
        for (size_t i = R.const0; i < R.const1; i++) {
            const SpellFold& f = P.cfolds[i];
            const uint32_t leaf = (uint32_t)(f.src / g.cs);
            CHECK(f.elided && g.leaves[leaf].elided && f.enc == g.leaves[leaf].enc && f.fbits == g.leaves[leaf].fbits);
            in_seg(paint(leaf, (uint32_t)(f.src % g.cs), f.nt, -1, -1, f.rows, f.cols, f.sr, f.init, f.dt, f.o_off, f.s_off, f.psz, f.lo, f.hi, f.flags, false));
            want_stats[PIECE_CONST] += (uint64_t)f.nt * f.rows * f.cols;
        }
        for (size_t i = R.unit0; i < R.unit1; i++) {
            const SpellUnit& u = P.units[i];
            const PlanLeaf& L = g.leaves[u.chunk];
            CHECK(!L.elided && L.bulk_ok && u.rr % 64 == 0 && u.rc % 64 == 0);
            CHECK(u.rr <= u.top && u.top < u.bottom && u.bottom <= u.rr + 64 && u.rc <= u.left && u.left < u.right && u.right <= u.rc + 64);
            const uint32_t ti = u.chunk / g.ntj % g.nti, tj = u.chunk % g.ntj;
            in_seg(paint(u.chunk, u.t0, u.t1 - u.t0, (int64_t)ti * g.tile + u.top - L.row0, (int64_t)tj * g.tile + u.left - L.col0, u.bottom - u.top,
                         u.right - u.left, u.sr, u.init, u.dt, u.o_off, u.s_off, u.psz, u.lo, u.hi, u.flags, true));
            want_stats[PIECE_BULK] += (uint64_t)(u.t1 - u.t0) * (u.bottom - u.top) * (u.right - u.left);
        }
        for (size_t s = R.slab0; s < R.slab1; s++) {
            const Slab& b = P.walk.slabs[s];
            uint64_t used = 0, item_cells = 0;
            for (size_t i = b.item0; i < b.item1; i++)
                item_cells += (uint64_t)(P.walk.items[i].bottom - P.walk.items[i].top) * (P.walk.items[i].right - P.walk.items[i].left);
            for (size_t i = b.fold0; i < b.fold1; i++) {
                const SpellFold& f = P.walk.folds[i];
                const uint64_t n = (uint64_t)f.nt * f.rows * f.cols;
                CHECK(f.src == used && !f.elided);
                used += n;
                // the fold's leaf, first instant and first cell, from the items that fill its block of the slab
                uint32_t leaf = 0, inst = ~0u, top = ~0u, left = ~0u;
                for (size_t j = b.item0; j < b.item1; j++) {
                    const WinItem& it = P.walk.items[j];
                    if (it.out_off < f.src || it.out_off >= f.src + n) continue;
                    CHECK(inst == ~0u || leaf == it.chunk);
                    leaf = it.chunk;
                    inst = std::min(inst, it.inst);
                    top = std::min<uint32_t>(top, it.top);
                    left = std::min<uint32_t>(left, it.left);
                }
                CHECK(inst != ~0u);
                const PlanLeaf& L = g.leaves[leaf];
                CHECK(!L.elided && !L.bulk_ok && f.enc == L.enc && f.fbits == L.fbits);
                const uint32_t ti = leaf / g.ntj % g.nti, tj = leaf % g.ntj;
                in_seg(paint(leaf, inst, f.nt, (int64_t)ti * g.tile + top - L.row0, (int64_t)tj * g.tile + left - L.col0, f.rows, f.cols, f.sr, f.init, f.dt,
                             f.o_off, f.s_off, f.psz, f.lo, f.hi, f.flags, false));
                want_stats[PIECE_WALK] += n;
            }
            CHECK(used == item_cells && used <= P.walk.slab_max);
            CHECK(used <= slab_cap || (b.fold1 - b.fold0 == 1 && P.walk.folds[b.fold0].nt == 1));
        }
        CHECK(seg_of > prev_seg);  // segments ascend, one per range
        prev_seg = seg_of;
    }
    CHECK(a_unit == P.units.size() && a_const == P.cfolds.size() && a_slab == P.walk.slabs.size());
    for (size_t q = 0; q < nq; q++)
        for (uint32_t nx : next[q]) CHECK(nx == nc[q].end - nc[q].start);  // every instant of every cell
    for (int k = 0; k < 3; k++) CHECK(P.stats[k] == want_stats[k]);
    return records;
}
static uint64_t check_plan() {
    uint64_t records = 0;
    const double inf = __builtin_inf();
    for (int geo = 0; geo < 4; geo++) {
        Geo G = geo < 3 ? plain(geo) : tiled();
        const uint32_t T = G.g.T, R = G.g.R, C = G.g.C;
        const dcdf_cube inner = geo < 3 ? dcdf_cube{1, 19, 33, 99, 63, 193} : dcdf_cube{1, 19, 5, 39, 20, 90};
        std::vector<dcdf_cube> cubes = {{0, T, 0, R, 0, C}, {T - 2, T - 1, R / 2, R / 2 + 1, C - 1, C}, {4, 4, 0, R, 0, C}, inner, {0, T, 7, 7, 1, C},
                                        {inner.end, inner.start, inner.bottom, inner.top, inner.right, inner.left}};
        std::vector<double> lower = {-3.5, 0.5, 1.0, 1099511627776.0, -inf, 2.25}, upper = {7.25, 0.5, 2.0, inf, inf, -100.0};
        std::vector<dcdf_cube> rev(cubes.rbegin(), cubes.rend());
        std::vector<double> rlo(lower.rbegin(), lower.rend()), rup(upper.rbegin(), upper.rend());
        for (int node_wise = 0; node_wise < 2; node_wise++)
            for (uint64_t slab : {(uint64_t)100, (uint64_t)1 << 22}) {
                records += check_plan_case(G, cubes, lower, upper, node_wise != 0, slab);
                records += check_plan_case(G, rev, rlo, rup, node_wise != 0, slab);
            }
    }
    // a NaN bound is refused
    Geo G = plain(0);
    G.g.leaves = G.leaves.data();
    const dcdf_cube c{0, 1, 0, 1, 0, 1};
    const double nan = __builtin_nan(""), zero = 0.0;
    const uint64_t b0 = 0;
    SpellPlan P((uint64_t)1 << 22);
    CHECK(plan_spells(G.g, &c, &nan, &zero, 1, &b0, &b0, true, P) == DCDF_ERR_BAD_ARG);
    CHECK(plan_spells(G.g, &c, &zero, &nan, 1, &b0, &b0, true, P) == DCDF_ERR_BAD_ARG);
    return records;
}

int main() {
    std::printf("ok cuts %" PRIu64 "\n", check_cuts());
    std::printf("ok hits %" PRIu64 "\n", check_hits());
    std::printf("ok plan %" PRIu64 "\n", check_plan());
    return 0;
}
