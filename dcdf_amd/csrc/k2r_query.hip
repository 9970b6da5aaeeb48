// k2r_query.hip -- C ABI, query side: get / fill_cell / fill_window / search on opened chunks (k2r_open.hip), single-chunk and
// batched.  Kernels walk the serialized big-endian bytes in HBM via k2r_decode.h; the raster layer (k2r_raster.hip) reaches them
// through the launchers of k2r_query_host.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "k2r_decode.h"
#include "k2r_query_host.h"

using namespace k2r;

namespace k2r {

// fill_window: one workgroup per query, threads stride over the window's cells; every cell is an
// independent root-to-leaf descent (block.rs:42-47), so writes are coalesced along columns.
__global__ void __launch_bounds__(256)
k_fill_window(const ChunkRef* __restrict__ chunks, const WinQuery* __restrict__ qs, uint32_t nq, void* out,
              int32_t out_dtype, int64_t st, int64_t sr, int64_t sc, int strided_single) {
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const WinQuery Q = qs[q];
        const ChunkRef C = chunks[Q.chunk];
        const uint32_t wr = Q.bottom - Q.top, wc = Q.right - Q.left, wt = Q.end - Q.start;
        const uint64_t cells = (uint64_t)wt * wr * wc;
        for (uint64_t e = threadIdx.x; e < cells; e += blockDim.x) {
            const uint32_t c = (uint32_t)(e % wc), r = (uint32_t)((e / wc) % wr), t = (uint32_t)(e / ((uint64_t)wc * wr));
            const int64_t v = inst_get(C.bytes, C.descs, Q.start + t, Q.top + r, Q.left + c);
            const int64_t off = strided_single ? (int64_t)t * st + (int64_t)r * sr + (int64_t)c * sc : (int64_t)(Q.out_off + e);
            store_typed(out, off, out_dtype, v, C.fbits);
        }
    }
}

// ---- wave-cooperative window decode ---------------------------------------------------------------------------------------
// fill_window the MI355X way: one WAVE per (query, instant, sub-window of at most 32 x 32 cells) walks the nodes that
// cover the sub-window ONCE, level by level (snapshot.rs:237-301, log.rs:349-508 are depth-first recursions over the same
// nodes): lane = (frontier node, child).  A node's rank / Dac hops are paid once per node instead of once per cell; the
// frontier lives in LDS and is compacted with ballot + mbcnt; uniform or "equal" subtrees become rectangle fills done by
// the whole wave; the last two levels (a node of side k and its cells) are finished by the lane that owns the node.
constexpr int WQ_CAP = 192;             // frontier entries per wave: nodes of side >= k^2 meeting a 32 x 32 window, all levels
struct WaveQ {
    uint32_t it[WQ_CAP], is[WQ_CAP], org[WQ_CAP];  // first child of the node in the log / snapshot tree (or NONE), origin row << 16 | col
    int64_t mt[WQ_CAP], ms[WQ_CAP];                 // log.rs:360-361 max_t, max_s
};
// One step of the synchronized descent (log.rs:392-505; snapshot.rs:281-299 when there is no log): child c of a node.
// Returns true when the child's whole square has one value (*val), else the child's state in *o.  The rank that locates
// the child's own children is computed HERE, next to the child's other loads (they are independent of each other), so that
// the next level does not start with a round trip of its own.
__device__ __forceinline__ bool window_child(const uint8_t* b, const InstDesc& S, const InstDesc* L, const NodeSt& p, uint32_t c,
                                             uint32_t k2, NodeSt* o, int64_t* val) {
    const bool has_t = p.bt != WQ_NONE, has_s = p.bs != WQ_NONE;
    const uint32_t it_ = has_t ? p.bt + c : 0u, is_ = has_s ? p.bs + c : 0u;
    const int64_t mt_ = has_t ? dacd_get(b, L->mx, it_) : p.mt;             // log.rs:397-400
    const int64_t ms_ = has_s ? p.ms - dacd_get(b, S.mx, is_) : p.ms;       // log.rs:412-415
    const bool leaf_t = has_t ? (it_ >= L->T.len || !bmd_get(b, L->T, it_)) : true;
    const bool leaf_s = has_s ? (is_ >= S.T.len || !bmd_get(b, S.T, is_)) : true;
    const uint32_t rt = has_t ? bmd_rank(b, L->T, it_) : 0u, rs = has_s ? bmd_rank(b, S.T, is_) : 0u;
    *val = mt_ + ms_;
    if (leaf_t && leaf_s) return true;
    o->mt = mt_;
    o->ms = ms_;
    if (leaf_s) {
        o->bt = 1 + rt * k2;
        o->bs = WQ_NONE;
        return false;
    }
    if (leaf_t) {
        // rank0(T, it_ + 1) - 1 with T[it_] == 0 is it_ - rank(T, it_)
        if (has_t && !bmd_get(b, L->E, it_ - rt)) return true;  // uniform, not "equal" (log.rs:452-467)
        o->bt = WQ_NONE;
        o->bs = 1 + rs * k2;
        return false;
    }
    o->bt = 1 + rt * k2;
    o->bs = 1 + rs * k2;
    return false;
}

__global__ void __launch_bounds__(256)
k_window_wave(const ChunkRef* __restrict__ chunks, const WinItem* __restrict__ items, uint32_t n_items, void* out, int32_t out_dtype) {
    __shared__ WaveQ wq[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WaveQ& q = wq[wave];
    for (uint32_t item = blockIdx.x * 4u + (uint32_t)wave; item < n_items; item += gridDim.x * 4u) {
        const WinItem I = items[item];
        const ChunkRef C = chunks[I.chunk];
        const uint8_t* const b = C.bytes;
        const InstDesc& D = C.descs[I.inst];
        const bool has_log = D.is_log != 0;
        const InstDesc& S = has_log ? C.descs[D.snap] : D;
        const InstDesc* const L = has_log ? &D : nullptr;
        const uint32_t k = D.k, k2 = k * k;
        const uint32_t wtop = I.top, wbot = I.bottom, wleft = I.left, wright = I.right;
        auto put = [&](uint32_t r, uint32_t c, int64_t v) {
            store_typed(out, (int64_t)I.out_off + (int64_t)(r - wtop) * I.out_sr + (c - wleft), out_dtype, v, C.fbits);
        };
        // rectangle [r0, r1) x [c0, c1) (already clipped to the sub-window) <- v, by the whole wave
        auto fill_wave = [&](uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, int64_t v) {
            const uint32_t w = c1 - c0, area = (r1 - r0) * w;
            for (uint32_t i = (uint32_t)lane; i < area; i += 64) put(r0 + i / w, c0 + i % w, v);
        };
        // ---- roots (snapshot.rs:211-219, log.rs:315-328) ----
        const bool single_s = !bmd_get(b, S.T, 0);
        const bool single_t = has_log ? !bmd_get(b, L->T, 0) : true;
        const int64_t max_s0 = dacd_get(b, S.mx, 0), max_t0 = has_log ? dacd_get(b, L->mx, 0) : 0;
        const bool all_one = has_log ? (single_t && (single_s || !bmd_get(b, L->E, 0))) : single_s;
        if (all_one) {
            fill_wave(wtop, wbot, wleft, wright, max_t0 + max_s0);
            continue;
        }
        if (lane == 0) {
            q.it[0] = (has_log && !single_t) ? 1u : WQ_NONE;  // children of the root start at 1 (rank(T, 0) == 0)
            q.is[0] = single_s ? WQ_NONE : 1u;
            q.org[0] = 0;
            q.mt[0] = max_t0;
            q.ms[0] = max_s0;
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t lo = 0, hi = 1, side = D.sidelen;
        const uint32_t per = 64u / k2;  // frontier nodes per step (lane = node * k2 + child)
        const uint32_t myn = (uint32_t)lane / k2, myc = (uint32_t)lane % k2;
        // ---- level by level while the children are still at least k x k ----
        while (side > k2) {
            const uint32_t cs = side / k;
            uint32_t next = hi;
            for (uint32_t base = lo; base < hi; base += per) {
                const uint32_t n = base + myn;
                const bool live = myn < per && n < hi;
                bool push = false, fill = false;
                NodeSt o{};
                int64_t val = 0;
                uint32_t r0 = 0, r1 = 0, c0 = 0, c1 = 0, org = 0;
                if (live) {
                    const NodeSt p{q.it[n], q.is[n], q.mt[n], q.ms[n]};
                    const uint32_t po = q.org[n];
                    const uint32_t cr = (po >> 16) + (myc / k) * cs, cc = (po & 0xffffu) + (myc % k) * cs;
                    r0 = cr > wtop ? cr : wtop; r1 = cr + cs < wbot ? cr + cs : wbot;
                    c0 = cc > wleft ? cc : wleft; c1 = cc + cs < wright ? cc + cs : wright;
                    if (r0 < r1 && c0 < c1) {
                        fill = window_child(b, S, L, p, myc, k2, &o, &val);
                        push = !fill;
                        org = (cr << 16) | cc;
                    }
                }
                const unsigned long long bp = __builtin_amdgcn_ballot_w64(push);
                if (push) {
                    const uint32_t pos = next + __builtin_amdgcn_mbcnt_hi((uint32_t)(bp >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bp, 0u));
                    if (pos < (uint32_t)WQ_CAP) {
                        q.it[pos] = o.bt; q.is[pos] = o.bs; q.org[pos] = org; q.mt[pos] = o.mt; q.ms[pos] = o.ms;
                    }
                }
                next += (uint32_t)__builtin_popcountll(bp);
                // fills: small ones by their lane, the others by the wave
                const bool small = (r1 - r0) * (c1 - c0) <= 4;
                if (fill && small)
                    for (uint32_t r = r0; r < r1; r++)
                        for (uint32_t c = c0; c < c1; c++) put(r, c, val);
                unsigned long long bf = __builtin_amdgcn_ballot_w64(fill && !small);
                while (bf) {
                    const int l = __builtin_ctzll(bf);
                    bf &= bf - 1;
                    const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)((r0 << 16) | r1), l);
                    const uint32_t cc = (uint32_t)__builtin_amdgcn_readlane((int)((c0 << 16) | c1), l);
                    const uint32_t vlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)val, l);
                    const uint32_t vhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)val >> 32), l);
                    fill_wave(rr >> 16, rr & 0xffffu, cc >> 16, cc & 0xffffu, (int64_t)(((uint64_t)vhi << 32) | vlo));
                }
            }
            __builtin_amdgcn_wave_barrier();
            lo = hi;
            hi = next < (uint32_t)WQ_CAP ? next : (uint32_t)WQ_CAP;  // (cannot overflow for sub-windows of <= 32 x 32: see the host)
            side = cs;
        }
        // ---- the last two levels: lane = (node of side <= k^2, child); the child's cells are finished by the lane ----
        {
            const uint32_t cs = side / k;  // k (then the grandchildren are cells) or 1 (the children are cells)
            for (uint32_t base = lo; base < hi; base += per) {
                const uint32_t n = base + myn;
                if (!(myn < per && n < hi)) continue;
                const NodeSt p{q.it[n], q.is[n], q.mt[n], q.ms[n]};
                const uint32_t po = q.org[n];
                const uint32_t cr = (po >> 16) + (myc / k) * cs, cc = (po & 0xffffu) + (myc % k) * cs;
                const uint32_t r0 = cr > wtop ? cr : wtop, r1 = cr + cs < wbot ? cr + cs : wbot;
                const uint32_t c0 = cc > wleft ? cc : wleft, c1 = cc + cs < wright ? cc + cs : wright;
                if (!(r0 < r1 && c0 < c1)) continue;
                NodeSt o{};
                int64_t val = 0;
                const bool fill = window_child(b, S, L, p, myc, k2, &o, &val);
                if (fill || cs == 1) {  // (a cell is always a leaf of both trees)
                    for (uint32_t r = r0; r < r1; r++)
                        for (uint32_t c = c0; c < c1; c++) put(r, c, val);
                    continue;
                }
                if (cs != k) {  // sidelen not a power of k (malformed input): plain per-cell descents
                    for (uint32_t r = r0; r < r1; r++)
                        for (uint32_t c = c0; c < c1; c++) put(r, c, inst_get(b, C.descs, I.inst, r, c));
                    continue;
                }
                if (k == 2) {  // the four cells at once: their loads are independent of each other
                    int64_t v[4];
                    NodeSt oo{};
#pragma unroll
                    for (int g = 0; g < 4; g++) (void)window_child(b, S, L, o, (uint32_t)g, k2, &oo, &v[g]);
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const uint32_t r = cr + (uint32_t)(g >> 1), c = cc + (uint32_t)(g & 1);
                        if (r >= r0 && r < r1 && c >= c0 && c < c1) put(r, c, v[g]);
                    }
                    continue;
                }
                for (uint32_t r = r0; r < r1; r++)
                    for (uint32_t c = c0; c < c1; c++) {
                        NodeSt oo{};
                        int64_t v = 0;
                        (void)window_child(b, S, L, o, (r - cr) * k + (c - cc), k2, &oo, &v);
                        put(r, c, v);
                    }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}


// ---- pruned search, any arity with k * k <= 64 -------------------------------------------------------------------------
// The reference's search is a pruned descent (snapshot.rs:347-421, log.rs:553-702): a subtree whose [min, max] misses [lower, upper]
// is skipped, one that lies inside is reported whole.  The same walk as k_window_wave -- lane = (frontier node, child), level by
// level, frontier in LDS -- carrying the node's exact extremes: max_t = Lmax_t + max_s as the window walk has it, and
// min_t = Lmin_t[rank(T_t, i)] + min_s for a node that is internal in the log (log.rs:148), min_s + (max_t - max_s) where the log
// is "equal" or has ended (t = s + constant there), with min_s carried down the snapshot (Lmin_s[rank(T_s, i)] = child_min -
// parent_min for internal nodes, snapshot.rs:140; min = max for its leaves).  Matches are bits of the search item's flat window
// bitmap.  The result set is the reference's wherever its bounds are true bounds; the one shape where they are not (SearchExtra:
// single-node uniform log over a multi-node snapshot) is evaluated as the data it is, on the snapshot with the root's difference.
struct SearchSt {
    uint32_t bt, bs;
    int64_t mt, ms, mns;  // max_t - max_s so far / max_s / min_s of the node
};
struct WaveQS {
    uint32_t it[WQ_CAP], is[WQ_CAP], org[WQ_CAP];
    int64_t mt[WQ_CAP], ms[WQ_CAP], mns[WQ_CAP];
};
// child c of node p: true = the child's square holds ONE value (*mx); else its state in *o and its extremes in *mn / *mx
__device__ __forceinline__ bool search_child(const uint8_t* b, const InstDesc& S, const InstDesc* L, const SearchSt& p, uint32_t c, uint32_t k2,
                                             SearchSt* o, int64_t* mn, int64_t* mx) {
    const bool has_t = p.bt != WQ_NONE, has_s = p.bs != WQ_NONE;
    const uint32_t it_ = has_t ? p.bt + c : 0u, is_ = has_s ? p.bs + c : 0u;
    const int64_t mt_ = has_t ? dacd_get(b, L->mx, it_) : p.mt;
    const int64_t ms_ = has_s ? p.ms - dacd_get(b, S.mx, is_) : p.ms;
    const bool leaf_t = has_t ? (it_ >= L->T.len || !bmd_get(b, L->T, it_)) : true;
    const bool leaf_s = has_s ? (is_ >= S.T.len || !bmd_get(b, S.T, is_)) : true;
    const uint32_t rt = has_t ? bmd_rank(b, L->T, it_) : 0u, rs = has_s ? bmd_rank(b, S.T, is_) : 0u;
    const int64_t mns_ = has_s ? (leaf_s ? ms_ : p.mns + dacd_get(b, S.mn, rs)) : p.mns;
    *mx = mt_ + ms_;
    *mn = (has_t && !leaf_t) ? dacd_get(b, L->mn, rt) + mns_ : mt_ + mns_;
    if (leaf_t && leaf_s) return true;
    o->mt = mt_;
    o->ms = ms_;
    o->mns = mns_;
    if (leaf_s) {
        o->bt = 1 + rt * k2;
        o->bs = WQ_NONE;
        return false;
    }
    if (leaf_t) {
        if (has_t && !bmd_get(b, L->E, it_ - rt)) return true;  // uniform, not "equal" (log.rs:452-467)
        o->bt = WQ_NONE;
        o->bs = 1 + rs * k2;
        return false;
    }
    o->bt = 1 + rt * k2;
    o->bs = 1 + rs * k2;
    return false;
}
// VALUE: a value search (dcdf_*_search_values): [lower, upper] are the stored integers value_bounds gave, the reference quirk is
// off (the true values are searched) and SearchExtra::quirk carries the hole instead: stored 0 inside the range is no match, so
// no subtree whose range holds 0 is taken whole.
template <bool VALUE = false>
__global__ void __launch_bounds__(256)
k_search_wave(const ChunkRef* __restrict__ chunks, const WinItem* __restrict__ items, uint32_t n_items, const SearchExtra* __restrict__ sx,
              uint32_t* __restrict__ bits, uint32_t* __restrict__ counts) {
    __shared__ WaveQS wq[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WaveQS& q = wq[wave];
    for (uint32_t item = blockIdx.x * 4u + (uint32_t)wave; item < n_items; item += gridDim.x * 4u) {
        const WinItem I = items[item];
        const SearchExtra X = sx[item];
        const ChunkRef C = chunks[I.chunk];
        const uint8_t* const b = C.bytes;
        const InstDesc& D = C.descs[I.inst];
        const bool quirk = !VALUE && X.quirk != 0;
        const bool has_log = D.is_log != 0 && !quirk;
        const InstDesc& S = D.is_log != 0 ? C.descs[D.snap] : D;
        const InstDesc* const L = has_log ? &D : nullptr;
        const uint32_t k = D.k, k2 = k * k;
        const uint32_t wtop = I.top, wbot = I.bottom, wleft = I.left, wright = I.right;
        const int64_t lower = X.lower, upper = X.upper;
        // (the integer instantiation's tests are exactly the plain comparisons)
        auto in_range = [&](int64_t v) {
            if constexpr (VALUE) return lower <= v && v <= upper && !(X.quirk != 0 && v == 0);
            else return lower <= v && v <= upper;
        };
        auto all_in = [&](int64_t mn, int64_t mx) {
            if constexpr (VALUE) return mn >= lower && mx <= upper && !(X.quirk != 0 && mn <= 0 && 0 <= mx);
            else return mn >= lower && mx <= upper;
        };
        uint32_t cnt = 0;
        // I.out_off = bit index of cell (top, left) in the item's flat window bitmap, I.out_sr = the window's width
        auto mark = [&](uint32_t r, uint32_t c) {
            const uint64_t e = I.out_off + (uint64_t)(r - wtop) * I.out_sr + (c - wleft);
            atomicOr(&bits[e >> 5], 1u << (e & 31u));
            cnt++;
        };
        auto mark_wave = [&](uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1) {
            const uint32_t w = c1 - c0, area = (r1 - r0) * w;
            for (uint32_t i = (uint32_t)lane; i < area; i += 64) mark(r0 + i / w, c0 + i % w);
        };
        // ---- roots ----
        const bool single_s = !bmd_get(b, S.T, 0);
        const bool single_t = has_log ? !bmd_get(b, L->T, 0) : true;
        const int64_t max_s0 = dacd_get(b, S.mx, 0), min_s0 = single_s ? max_s0 : dacd_get(b, S.mn, 0);  // (a leaf root has no Lmin entry)
        int64_t max_t0 = has_log ? dacd_get(b, L->mx, 0) : 0;
        bool done = false;
        if (quirk) {  // (log.rs:527-586 on this shape: SearchExtra)
            const int64_t c1 = dacd_get(b, D.mx, 0) + max_s0;
            if (min_s0 >= lower && c1 <= upper) {
                mark_wave(wtop, wbot, wleft, wright);
                done = true;
            } else if (min_s0 > upper || c1 < lower) {
                done = true;
            }
            max_t0 = c1 - max_s0;  // the walk below: s(cell) + (c - max_s(root))
        } else {
            const bool all_one = has_log ? (single_t && (single_s || !bmd_get(b, L->E, 0))) : single_s;
            if (all_one) {
                const int64_t v = max_t0 + max_s0;
                if (in_range(v)) mark_wave(wtop, wbot, wleft, wright);
                done = true;
            }
        }
        if (!done) {
            if (lane == 0) {
                q.it[0] = (has_log && !single_t) ? 1u : WQ_NONE;
                q.is[0] = single_s ? WQ_NONE : 1u;
                q.org[0] = 0;
                q.mt[0] = max_t0;
                q.ms[0] = max_s0;
                q.mns[0] = min_s0;
            }
            __builtin_amdgcn_wave_barrier();
            uint32_t lo = 0, hi = 1, side = D.sidelen;
            const uint32_t per = 64u / k2;
            const uint32_t myn = (uint32_t)lane / k2, myc = (uint32_t)lane % k2;
            while (side > k2) {
                const uint32_t cs = side / k;
                uint32_t next = hi;
                for (uint32_t base = lo; base < hi; base += per) {
                    const uint32_t n = base + myn;
                    const bool live = myn < per && n < hi;
                    bool push = false, fill = false;
                    SearchSt o{};
                    uint32_t r0 = 0, r1 = 0, c0 = 0, c1 = 0, org = 0;
                    if (live) {
                        const SearchSt p{q.it[n], q.is[n], q.mt[n], q.ms[n], q.mns[n]};
                        const uint32_t po = q.org[n];
                        const uint32_t cr = (po >> 16) + (myc / k) * cs, cc = (po & 0xffffu) + (myc % k) * cs;
                        r0 = cr > wtop ? cr : wtop; r1 = cr + cs < wbot ? cr + cs : wbot;
                        c0 = cc > wleft ? cc : wleft; c1 = cc + cs < wright ? cc + cs : wright;
                        if (r0 < r1 && c0 < c1) {
                            int64_t mn = 0, mx = 0;
                            const bool one = search_child(b, S, L, p, myc, k2, &o, &mn, &mx);
                            if (one) fill = in_range(mx);
                            else if (mx < lower || mn > upper) fill = false;      // nothing of this subtree is in range
                            else if (all_in(mn, mx)) fill = true;                 // all of it is
                            else push = true;
                            org = (cr << 16) | cc;
                        }
                    }
                    const unsigned long long bp = __builtin_amdgcn_ballot_w64(push);
                    if (push) {
                        const uint32_t pos = next + __builtin_amdgcn_mbcnt_hi((uint32_t)(bp >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bp, 0u));
                        if (pos < (uint32_t)WQ_CAP) {
                            q.it[pos] = o.bt; q.is[pos] = o.bs; q.org[pos] = org; q.mt[pos] = o.mt; q.ms[pos] = o.ms; q.mns[pos] = o.mns;
                        }
                    }
                    next += (uint32_t)__builtin_popcountll(bp);
                    const bool small = (r1 - r0) * (c1 - c0) <= 4;
                    if (fill && small)
                        for (uint32_t r = r0; r < r1; r++)
                            for (uint32_t c = c0; c < c1; c++) mark(r, c);
                    unsigned long long bf = __builtin_amdgcn_ballot_w64(fill && !small);
                    while (bf) {
                        const int l = __builtin_ctzll(bf);
                        bf &= bf - 1;
                        const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)((r0 << 16) | r1), l);
                        const uint32_t cc = (uint32_t)__builtin_amdgcn_readlane((int)((c0 << 16) | c1), l);
                        mark_wave(rr >> 16, rr & 0xffffu, cc >> 16, cc & 0xffffu);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                lo = hi;
                hi = next < (uint32_t)WQ_CAP ? next : (uint32_t)WQ_CAP;
                side = cs;
            }
            // ---- the last two levels ----
            {
                const uint32_t cs = side / k;
                for (uint32_t base = lo; base < hi; base += per) {
                    const uint32_t n = base + myn;
                    if (!(myn < per && n < hi)) continue;
                    const SearchSt p{q.it[n], q.is[n], q.mt[n], q.ms[n], q.mns[n]};
                    const uint32_t po = q.org[n];
                    const uint32_t cr = (po >> 16) + (myc / k) * cs, cc = (po & 0xffffu) + (myc % k) * cs;
                    const uint32_t r0 = cr > wtop ? cr : wtop, r1 = cr + cs < wbot ? cr + cs : wbot;
                    const uint32_t c0 = cc > wleft ? cc : wleft, c1 = cc + cs < wright ? cc + cs : wright;
                    if (!(r0 < r1 && c0 < c1)) continue;
                    SearchSt o{};
                    int64_t mn = 0, mx = 0;
                    const bool one = search_child(b, S, L, p, myc, k2, &o, &mn, &mx);
                    if (one || cs == 1) {  // (a cell is always a leaf of both trees)
                        if (in_range(mx))
                            for (uint32_t r = r0; r < r1; r++)
                                for (uint32_t c = c0; c < c1; c++) mark(r, c);
                        continue;
                    }
                    if (mx < lower || mn > upper) continue;
                    if (all_in(mn, mx)) {
                        for (uint32_t r = r0; r < r1; r++)
                            for (uint32_t c = c0; c < c1; c++) mark(r, c);
                        continue;
                    }
                    const int64_t shift = quirk ? max_t0 : 0;  // (per-cell descents below decode the true instant; the quirk walks the snapshot)
                    if (cs != k) {  // sidelen not a power of k (malformed input): plain per-cell descents
                        for (uint32_t r = r0; r < r1; r++)
                            for (uint32_t c = c0; c < c1; c++) {
                                const int64_t v = inst_get(b, C.descs, quirk ? D.snap : I.inst, r, c) + shift;
                                if (in_range(v)) mark(r, c);
                            }
                        continue;
                    }
                    for (uint32_t r = r0; r < r1; r++)
                        for (uint32_t c = c0; c < c1; c++) {
                            SearchSt oo{};
                            int64_t vn = 0, v = 0;
                            (void)search_child(b, S, L, o, (r - cr) * k + (c - cc), k2, &oo, &vn, &v);
                            if (in_range(v)) mark(r, c);
                        }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // the item's count: this wave's matches, summed over its lanes
        for (int o2 = 32; o2 > 0; o2 >>= 1) cnt += __shfl_down(cnt, o2, 64);
        if (lane == 0 && cnt) atomicAdd(&counts[X._pad], cnt);
    }
}

// What a search item adds to its WinItem (search = the same walk; instead of storing a cell it tests lower <= v <= upper and
// sets the cell's bit in the item's own bitmap -- 64 rows x 2 words: word = 2 * (row - top) + (column - left) / 32 -- at out[item * 128];
// no two waves share a word, so there is nothing atomic about it and nothing to clear beforehand).
// MW = waves per SIMD the register allocator must leave room for (4 for the 32-bit walk; the 64-bit one's frontier leaves LDS
// for 3 workgroups per CU, so it is built for 3); DENSE64: the batched form's output (int64, unit column stride);
// SEARCH: mark matches (out = the bitmaps, sx = one SearchExtra per item) instead of storing values
// VALUE (with SEARCH): a value search, as in k_search_wave: no quirk, SearchExtra::quirk is the hole.  (A raster piece whose bounds
// translate to no stored integer comes as [INT64_MAX, INT64_MIN]: every side-16 square is skipped at once.  An early exit for it
// here costs 18 VGPRs and spills this walk's 64-bit form.)
template <int MW, bool DENSE64, bool SEARCH = false, class V = int64_t, bool USE_TOP = true, bool VALUE = false>
__global__ void __launch_bounds__(256, MW)
k_window_wave2(const ChunkRef* __restrict__ chunks, const WinItem* __restrict__ items, uint32_t n_items, void* out, int32_t out_dtype,
               const SearchExtra* __restrict__ sx = nullptr) {
    typedef NodeStT<V> NodeSt;
    typedef KidsT<V> Kids;
    __shared__ WaveQ2T<V> wq[4];
    __shared__ uint32_t wbits[4][128];  // SEARCH: the item's matches, two words per row (bit = column - wleft)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WaveQ2T<V>& q = wq[wave];
    uint32_t* const rowbits = wbits[wave];
    for (uint32_t item = blockIdx.x * 4u + (uint32_t)wave; item < n_items; item += gridDim.x * 4u) {
        const WinItem I = items[item];
        const ChunkRef C = chunks[I.chunk];
        const uint8_t* const b = C.bytes;
        const gbytes gb = (gbytes)C.bytes;
        const gdesc gD = (gdesc)C.descs + I.inst;
        const bool has_log = gD->is_log != 0;
        const gdesc gS = has_log ? (gdesc)C.descs + gD->snap : gD;
        const InstDesc& D = C.descs[I.inst];                       // (generic views: only for the rare general Dac walk)
        const InstDesc& SD = has_log ? C.descs[gD->snap] : D;
        const TreeRef S = tree_ref(gS), L = tree_ref(gD);          // (L is only looked at when has_log)
        const uint32_t sidelen0 = gD->sidelen;
        const uint32_t wtop = I.top, wbot = I.bottom, wleft = I.left, wright = I.right, osr = I.out_sr;
        const int64_t obase = (int64_t)I.out_off - (int64_t)wtop * osr - (int64_t)wleft;  // element offset of chunk cell (0, 0)
        int64_t s_lo = 0, s_hi = 0;
        bool quirk = false, hole = false;
        if (SEARCH) {
            s_lo = sx[item].lower;
            s_hi = sx[item].upper;
            if constexpr (VALUE) hole = __builtin_amdgcn_readfirstlane((int)sx[item].quirk) != 0;
            else quirk = __builtin_amdgcn_readfirstlane((int)sx[item].quirk) != 0;
            rowbits[2 * lane] = 0;
            rowbits[2 * lane + 1] = 0;
            __builtin_amdgcn_wave_barrier();
        }
        auto put = [&](uint32_t r, uint32_t c, int64_t v) {
            if (SEARCH) {
                const uint32_t j = c - wleft;
                if constexpr (VALUE) {
                    if (s_lo <= v && v <= s_hi && !(hole && v == 0)) atomicOr(&rowbits[2 * (r - wtop) + (j >> 5)], 1u << (j & 31u));
                } else {
                    if (s_lo <= v && v <= s_hi) atomicOr(&rowbits[2 * (r - wtop) + (j >> 5)], 1u << (j & 31u));
                }
                return;
            }
            const int64_t off = obase + (int64_t)(r * osr + c);
            if (DENSE64) ((int64_t*)out)[off] = v;
            else store_typed(out, off, out_dtype, v, C.fbits);
        };
        auto flush_bits = [&]() {
            if (!SEARCH) return;
            __builtin_amdgcn_wave_barrier();
            ((uint32_t*)out)[(uint64_t)item * 128u + 2u * (uint32_t)lane] = rowbits[2 * lane];  // (rows beyond the item: 0)
            ((uint32_t*)out)[(uint64_t)item * 128u + 2u * (uint32_t)lane + 1u] = rowbits[2 * lane + 1];
            __builtin_amdgcn_wave_barrier();
        };
        auto fill_wave = [&](uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, int64_t v) {
            if (SEARCH) {  // (v is wave-uniform) a rectangle of one value: whole row segments at once
                bool hit = s_lo <= v && v <= s_hi;
                if constexpr (VALUE) hit = hit && !(hole && v == 0);
                if (hit && (uint32_t)lane < r1 - r0 && c1 > c0) {
                    const uint32_t w1 = c1 - c0;
                    const uint64_t m = (w1 >= 64u ? ~0ull : ((1ull << w1) - 1ull)) << (c0 - wleft);
                    uint32_t* const rw = &rowbits[2 * (r0 - wtop + (uint32_t)lane)];
                    if ((uint32_t)m) atomicOr(rw, (uint32_t)m);
                    if ((uint32_t)(m >> 32)) atomicOr(rw + 1, (uint32_t)(m >> 32));
                }
                return;
            }
            const uint32_t w = c1 - c0, area = (r1 - r0) * w;
            if (w <= 32 && area <= 1024) {                             // (every fill below the top table)
                const uint32_t inv = (65536u + w - 1) / w;             // i / w == (i * inv) >> 16 for i < 2048
                for (uint32_t i = (uint32_t)lane; i < area; i += 64) {
                    const uint32_t rr = (i * inv) >> 16;
                    put(r0 + rr, c0 + i - rr * w, v);
                }
            } else {
                for (uint32_t i = (uint32_t)lane; i < area; i += 64) put(r0 + i / w, c0 + i % w, v);
            }
        };
        uint32_t lo = 0, hi = 1, side = sidelen0;
        if (USE_TOP && C.top && !(SEARCH && quirk)) {  // start at the (up to 5 x 5) nodes of side 16 that meet the item (k_top_table)
            typedef __attribute__((address_space(1))) const TopEnt* gtop;
            const uint32_t r16 = wtop >> 4, c16 = wleft >> 4, nr16 = ((wbot - 1u) >> 4) - r16 + 1u, nc16 = ((wright - 1u) >> 4) - c16 + 1u;  // <= 5 each
            const uint32_t qi = (uint32_t)lane / nc16, qj = (uint32_t)lane - qi * nc16;
            const uint32_t cr = (r16 + qi) << 4, cc = (c16 + qj) << 4;
            const bool mine = (uint32_t)lane < nr16 * nc16;
            uint32_t ebt = WQ_NONE, ebs = WQ_NONE;
            int64_t emt = 0, ems = 0;
            if (mine) {
                const gtop e = (gtop)C.top + ((size_t)I.inst * C.top_g + (cr >> 4)) * C.top_g + (cc >> 4);
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 x = *(__attribute__((address_space(1))) const u32x4*)e;
                ebt = x.x; ebs = x.y; emt = (int32_t)x.z; ems = (int32_t)x.w;
            }
            // search: the square's value range decides without a descent when it lies outside or inside [lower, upper]
            // (the reference prunes the same way at every node, log.rs:575-586; here once, at side 16)
            bool skip = false, force = false;
            if (SEARCH && mine) {
                typedef __attribute__((address_space(1))) const TopMM* gmm;
                const gmm m = (gmm)C.top_mm + ((size_t)I.inst * C.top_g + (cr >> 4)) * C.top_g + (cc >> 4);
                const int64_t vmin = m->vmin, vmax = m->vmax;
                skip = vmax < s_lo || vmin > s_hi;
                force = !skip && s_lo <= vmin && vmax <= s_hi;
                if constexpr (VALUE) force = force && !(hole && vmin <= 0 && 0 <= vmax);  // (the hole is inside: descend)
            }
            const bool isfill = mine && !skip && !force && ebt == WQ_NONE && ebs == WQ_NONE;
            const bool push = mine && !skip && !force && !isfill;
            if (SEARCH) {
                unsigned long long bo = __builtin_amdgcn_ballot_w64(force);
                while (bo) {  // every cell of the square matches: its part of the sub-window at once
                    const int l = __builtin_ctzll(bo);
                    bo &= bo - 1;
                    const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)cr, l), ccl = (uint32_t)__builtin_amdgcn_readlane((int)cc, l);
                    fill_wave(rr > wtop ? rr : wtop, rr + 16 < wbot ? rr + 16 : wbot, ccl > wleft ? ccl : wleft, ccl + 16 < wright ? ccl + 16 : wright, s_lo);
                }
            }
            const unsigned long long bp = __builtin_amdgcn_ballot_w64(push);
            if (push) {
                const uint32_t pos = __builtin_amdgcn_mbcnt_lo((uint32_t)bp, 0u);
                q.it[pos] = ebt; q.is[pos] = ebs; q.org[pos] = (cr << 16) | cc; q.mt[pos] = (V)emt; q.ms[pos] = (V)ems;
            }
            unsigned long long bf = __builtin_amdgcn_ballot_w64(isfill);
            while (bf) {  // squares of one value: their part of the sub-window, by the whole wave
                const int l = __builtin_ctzll(bf);
                bf &= bf - 1;
                const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)cr, l), ccl = (uint32_t)__builtin_amdgcn_readlane((int)cc, l);
                const int64_t v = (int64_t)__builtin_amdgcn_readlane((int)(int32_t)emt, l) + (int64_t)__builtin_amdgcn_readlane((int)(int32_t)ems, l);
                fill_wave(rr > wtop ? rr : wtop, rr + 16 < wbot ? rr + 16 : wbot, ccl > wleft ? ccl : wleft, ccl + 16 < wright ? ccl + 16 : wright, v);
            }
            hi = (uint32_t)__builtin_popcountll(bp);
            side = 16;
            if (hi == 0) {
                flush_bits();
                continue;
            }
        } else {
            const bool single_s = !gbm_get(gb, S.T, 0);
            const bool single_t = has_log ? !gbm_get(gb, L.T, 0) : true;
            const int64_t max_s0 = dacd_get(b, SD.mx, 0), max_t0 = has_log ? dacd_get(b, D.mx, 0) : 0;
            const bool all_one = has_log ? (single_t && (single_s || !gbm_get(gb, L.E, 0))) : single_s;
            if (SEARCH && quirk) {  // (see SearchExtra: the reference's result for this shape, log.rs:527-586)
                const int64_t min_s0 = dacd_get(b, SD.mn, 0), c1 = max_t0 + max_s0;
                if (min_s0 >= s_lo && c1 <= s_hi) {
                    fill_wave(wtop, wbot, wleft, wright, s_lo);  // every cell
                    flush_bits();
                    continue;
                }
                if (min_s0 > s_hi || c1 < s_lo) {
                    flush_bits();
                    continue;
                }
                // else: the snapshot's tree with the root's difference on top of every value (the walk below, it = NONE)
            } else if (all_one) {
                fill_wave(wtop, wbot, wleft, wright, max_t0 + max_s0);
                flush_bits();
                continue;
            }
            if (lane == 0) {
                q.it[0] = (has_log && !single_t) ? 1u : WQ_NONE;
                q.is[0] = single_s ? WQ_NONE : 1u;
                q.org[0] = 0;
                q.mt[0] = (V)max_t0;
                q.ms[0] = (V)max_s0;
            }
        }
        __builtin_amdgcn_wave_barrier();
        while (side > 4) {  // lane = frontier node; children of side >= 4 go to the next frontier
            const uint32_t cs = side >> 1;
            uint32_t next = hi;
            for (uint32_t base = lo; base < hi; base += 64) {
                const uint32_t n = base + (uint32_t)lane;
                const bool live = n < hi;
                Kids kd;
                kd.fill = 0;
                uint32_t po = 0, inter = 0;  // children meeting the sub-window
                if (live) {
                    const NodeSt p{q.it[n], q.is[n], q.mt[n], q.ms[n]};
                    po = q.org[n];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const uint32_t cr = (po >> 16) + (uint32_t)(c >> 1) * cs, cc = (po & 0xffffu) + (uint32_t)(c & 1) * cs;
                        if (cr < wbot && cr + cs > wtop && cc < wright && cc + cs > wleft) inter |= 1u << c;
                    }
                    if (inter) expand4(gb, S, SD.mx, L, D.mx, p, &kd);
                }
                const uint32_t pushm = inter & ~kd.fill, fillm = inter & kd.fill;
                const uint32_t np = popc32(pushm);
                const uint32_t inc = GpuExecScan::incl(np);
                uint32_t pos = next + inc - np;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if ((pushm >> c) & 1u) {
                        if (pos < (uint32_t)WQ2_CAP) {
                            const uint32_t cr = (po >> 16) + (uint32_t)(c >> 1) * cs, cc = (po & 0xffffu) + (uint32_t)(c & 1) * cs;
                            q.it[pos] = kd.st[c].bt; q.is[pos] = kd.st[c].bs; q.org[pos] = (cr << 16) | cc; q.mt[pos] = kd.st[c].mt; q.ms[pos] = kd.st[c].ms;
                        }
                        pos++;
                    }
                next += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
#pragma unroll
                for (int c = 0; c < 4; c++) {  // uniform / not-"equal" children: their part of the sub-window, by the whole wave
                    unsigned long long bf = __builtin_amdgcn_ballot_w64((fillm >> c) & 1u);
                    const uint32_t cr = (po >> 16) + (uint32_t)(c >> 1) * cs, cc = (po & 0xffffu) + (uint32_t)(c & 1) * cs;
                    while (bf) {
                        const int l = __builtin_ctzll(bf);
                        bf &= bf - 1;
                        const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)cr, l), ccl = (uint32_t)__builtin_amdgcn_readlane((int)cc, l);
                        const uint32_t vlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)kd.val[c], l);
                        const uint32_t vhi = sizeof(V) == 4 ? (uint32_t)((int32_t)vlo >> 31)
                                                            : (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)(int64_t)kd.val[c] >> 32), l);
                        fill_wave(rr > wtop ? rr : wtop, rr + cs < wbot ? rr + cs : wbot, ccl > wleft ? ccl : wleft, ccl + cs < wright ? ccl + cs : wright,
                                  (int64_t)(((uint64_t)vhi << 32) | vlo));
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            lo = hi;
            hi = next < (uint32_t)WQ2_CAP ? next : (uint32_t)WQ2_CAP;
            side = cs;
        }
        // ---- nodes of side 4: the lane finishes its 16 cells ----
#ifdef K2R_DIAG_NO_FINAL
        hi = lo;  // (diagnostic build: time of the upper levels alone; results are wrong)
#endif
        // A lane expands one node of side 4 into its quads.  A quad of one value is written at once; the OPEN quads (two Dac
        // reads each, the expensive part) of all the lanes are compacted into the free tail of the frontier and then taken one
        // per lane: typically a third of the quads are open, so a lane-per-node loop over all four would spend two thirds of
        // its Dac reads on masked-off lanes.
        auto put_quad = [&](uint32_t cr, uint32_t cc, const V (&v)[4]) {
            const bool in = cr >= wtop && cr + 2 <= wbot && cc >= wleft && cc + 2 <= wright;
            if (DENSE64 && !SEARCH && in) {  // two cells of a row per store (16 bytes, any 8-byte alignment)
                typedef long long ll2 __attribute__((ext_vector_type(2)));
                typedef ll2 __attribute__((aligned(8))) ll2u;
                int64_t* const o0 = (int64_t*)out + (obase + (int64_t)(cr * osr + cc));
                *(__attribute__((address_space(1))) ll2u*)o0 = ll2{(long long)v[0], (long long)v[1]};
                *(__attribute__((address_space(1))) ll2u*)(o0 + osr) = ll2{(long long)v[2], (long long)v[3]};
                return;
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t r = cr + (uint32_t)(e >> 1), cl = cc + (uint32_t)(e & 1);
                if (in || (r >= wtop && r < wbot && cl >= wleft && cl < wright)) put(r, cl, v[e]);
            }
        };
        const uint32_t room = ((uint32_t)WQ2_CAP - hi) / 4u;            // nodes per round whose quads fit the tail
        const uint32_t per_round = room < 64u ? room : 64u;
        for (uint32_t base = lo; base < hi; base += (per_round ? per_round : 64u)) {
            const uint32_t n = base + (uint32_t)lane;
            const bool live = n < hi && (per_round == 0 || (uint32_t)lane < per_round);
            Kids kd;
            kd.fill = 0;
            uint32_t pr = 0, pc = 0, openm = 0;
            if (live) {
                const NodeSt p{q.it[n], q.is[n], q.mt[n], q.ms[n]};
                const uint32_t po = q.org[n];
                pr = po >> 16;
                pc = po & 0xffffu;
                expand4(gb, S, SD.mx, L, D.mx, p, &kd);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t cr = pr + 2u * (uint32_t)(c >> 1), cc = pc + 2u * (uint32_t)(c & 1);
                    if (!(cr < wbot && cr + 2 > wtop && cc < wright && cc + 2 > wleft)) continue;  // outside the item
                    if ((kd.fill >> c) & 1u) {
                        const V v[4] = {kd.val[c], kd.val[c], kd.val[c], kd.val[c]};
                        put_quad(cr, cc, v);
                    } else {
                        openm |= 1u << c;
                    }
                }
            }
            if (per_round == 0) {  // (no room in the frontier's tail: the lane finishes its own quads)
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if ((openm >> c) & 1u) {
                        Kids g;
                        expand4(gb, S, SD.mx, L, D.mx, kd.st[c], &g);
                        put_quad(pr + 2u * (uint32_t)(c >> 1), pc + 2u * (uint32_t)(c & 1), g.val);
                    }
                continue;
            }
            const uint32_t np = popc32(openm);
            const uint32_t inc = GpuExecScan::incl(np);
            uint32_t pos = hi + inc - np;
#pragma unroll
            for (int c = 0; c < 4; c++)
                if ((openm >> c) & 1u) {
                    q.it[pos] = kd.st[c].bt; q.is[pos] = kd.st[c].bs; q.mt[pos] = kd.st[c].mt; q.ms[pos] = kd.st[c].ms;
                    q.org[pos] = ((pr + 2u * (uint32_t)(c >> 1)) << 16) | (pc + 2u * (uint32_t)(c & 1));
                    pos++;
                }
            const uint32_t nopen = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            __builtin_amdgcn_wave_barrier();
            for (uint32_t kb = 0; kb < nopen; kb += 64) {  // one open quad per lane: its four cells (expand4 at the cell level:
                const uint32_t m = kb + (uint32_t)lane;     // log.rs:404-420, snapshot.rs:281-299)
                if (m < nopen) {
                    const NodeSt k{q.it[hi + m], q.is[hi + m], q.mt[hi + m], q.ms[hi + m]};
                    const uint32_t ko = q.org[hi + m];
                    const bool ht = k.bt != WQ_NONE, hs = k.bs != WQ_NONE;
                    V vt[4], vs[4], v[4];
                    dac4(gb, L, D.mx, ht ? k.bt : 0u, vt);  // (both unconditional: the two chains of loads are in flight together)
                    dac4(gb, S, SD.mx, hs ? k.bs : 0u, vs);
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = (ht ? vt[e] : k.mt) + (hs ? k.ms - vs[e] : k.ms);
                    put_quad(ko >> 16, ko & 0xffffu, v);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        flush_bits();
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void __launch_bounds__(64)
k_search_count(const uint32_t* __restrict__ wbits, const SearchItem* __restrict__ items, const WinQuery* __restrict__ qs, uint32_t n,
               uint32_t* __restrict__ counts) {
    const uint32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n) return;
    const SearchItem I = items[it];
    if (I.w0 == SI_FLAT) return;  // (counted by k_search_cells)
    const WinQuery Q = qs[I.query];
    counts[it] = search_count_wave_item(wbits, I, Q);
}

// get / fill_cell: one thread per (query) point
__global__ void __launch_bounds__(256)
k_get(const ChunkRef* __restrict__ chunks, const PointQuery* __restrict__ qs, uint32_t nq, int64_t* __restrict__ out) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const PointQuery Q = qs[q];
    const ChunkRef C = chunks[Q.chunk];
    out[q] = inst_get(C.bytes, C.descs, Q.instant, Q.row, Q.col);
}

// the same with explicit output positions (fill_cell batches: query q's series goes to out + out_offset[q])
__global__ void __launch_bounds__(256)
k_get_at(const ChunkRef* __restrict__ chunks, const PointQuery* __restrict__ qs, uint32_t nq, int64_t* __restrict__ out,
         const uint64_t* __restrict__ at) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const PointQuery Q = qs[q];
    const ChunkRef C = chunks[Q.chunk];
    out[at[q]] = inst_get(C.bytes, C.descs, Q.instant, Q.row, Q.col);
}

// search pass 1 for chunks the wave walk does not take (k != 2): decode and test.  One WAVE per (query, instant) item; the
// lanes stride over the window's cells, each a root-to-leaf descent (inst_get), and mark the cells in range in the item's flat
// window bitmap.  The reference's search is a pruned descent whose result is exactly that set (its bounds are true bounds) --
// except for the single-node-uniform-log shape of SearchExtra, which is evaluated here as the data it is: all cells, no cell, or
// the cells with lower <= s(cell) + (c - max_s(root)) <= upper.
// VALUE: a value search, as in k_search_wave (quirk[] holds the items' hole flags)
template <bool VALUE = false>
__global__ void __launch_bounds__(64)
k_search_cells(const ChunkRef* __restrict__ chunks, const WinQuery* __restrict__ qs, const SearchItem* __restrict__ items,
               uint32_t n_items, const uint8_t* __restrict__ quirk, uint32_t* __restrict__ bits, uint32_t* __restrict__ counts) {
    const uint32_t it = blockIdx.x;
    if (it >= n_items) return;
    const SearchItem I = items[it];
    if (I.w0 != SI_FLAT) return;  // (marked by the wave walk)
    const int lane = threadIdx.x;
    const WinQuery Q = qs[I.query];
    const ChunkRef C = chunks[Q.chunk];
    const uint8_t* const b = C.bytes;
    const uint32_t wc = Q.right - Q.left, ncell = (Q.bottom - Q.top) * wc;
    uint32_t* const bw = bits + I.bits_off;
    const InstDesc& D = C.descs[I.instant];
    bool all = false, none = false;
    int64_t shift = 0;
    uint32_t from = I.instant;
    bool hole = false;
    if constexpr (VALUE) hole = quirk[it] != 0;
    if (!VALUE && quirk[it]) {  // (log.rs:527-586 on this shape)
        const InstDesc& S = C.descs[D.snap];
        const int64_t max_s0 = dacd_get(b, S.mx, 0), min_s0 = dacd_get(b, S.mn, 0), c1 = dacd_get(b, D.mx, 0) + max_s0;
        all = min_s0 >= Q.lower && c1 <= Q.upper;
        none = !all && (min_s0 > Q.upper || c1 < Q.lower);
        shift = c1 - max_s0;
        from = D.snap;
    }
    uint32_t cnt = 0;
    if (!none) {
        for (uint32_t e = (uint32_t)lane; e < ncell; e += 64) {
            bool hit = all;
            if (!all) {
                const int64_t v = inst_get(b, C.descs, from, Q.top + e / wc, Q.left + e % wc) + shift;
                hit = Q.lower <= v && v <= Q.upper;
                if constexpr (VALUE) hit = hit && !(hole && v == 0);
            }
            if (hit) {
                atomicOr(&bw[e >> 5], 1u << (e & 31u));
                cnt++;
            }
        }
    }
    // wave total (DPP-free: a shuffle ladder is fine here)
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (lane == 0) counts[it] = cnt;
}
// search pass 2: expand the bitmaps into sorted (instant,row,col) triples
__global__ void __launch_bounds__(64)
k_search_emit(const WinQuery* __restrict__ qs, const SearchItem* __restrict__ items, uint32_t n_items,
              const uint32_t* __restrict__ bits, const uint32_t* __restrict__ wbits, const uint64_t* __restrict__ offs,
              uint32_t* __restrict__ out) {
    const uint32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_items) return;
    const SearchItem I = items[it];
    const WinQuery Q = qs[I.query];
    const uint32_t wc = Q.right - Q.left, nbits = (Q.bottom - Q.top) * wc;
    const uint32_t* bw = bits + I.bits_off;
    uint32_t* o = out + 3 * offs[it];
    // origin of the chunk inside its raster (dcdf_raster_search_batch; zero for chunk-level searches): a search does not use
    // out_off / _pad otherwise
    const uint32_t ot = Q._pad, orow = (uint32_t)Q.out_off, ocol = (uint32_t)(Q.out_off >> 32);
    if (I.w0 != SI_FLAT) {  // the pieces' bitmaps (64 rows x 2 words) of the wave walk: rows in order, pieces left to right
        search_emit_wave_item(I, Q, wbits, o);
        return;
    }
    for (uint32_t w = 0; w < (nbits + 31) / 32; w++) {
        uint32_t x = bw[w];
        while (x) {
            const uint32_t p = 32 * w + (uint32_t)__builtin_ctz(x);
            x &= x - 1;
            o[0] = ot + I.instant;
            o[1] = orow + Q.top + p / wc;
            o[2] = ocol + Q.left + p % wc;
            o += 3;
        }
    }
}

}  // namespace k2r

// ---- point queries --------------------------------------------------------------------------------------
// A host thread's page of pinned, device-visible memory: single get / short fill_cell calls put their queries there and the
// kernel writes the answers there -- no allocation and no explicit copy per call (the round-1 form did three hipMalloc, two
// H2D copies and one D2H copy per cell).
namespace {
struct PinnedPage {
    static constexpr size_t kPoints = 1024;
    ChunkRef* ref = nullptr;  // [1]
    PointQuery* q = nullptr;  // [kPoints]
    int64_t* out = nullptr;   // [kPoints]
    void* base = nullptr;
    bool init() {
        if (base) return true;
        const size_t bytes = 256 + kPoints * (sizeof(PointQuery) + 8);
        if (hipHostMalloc(&base, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            base = nullptr;
            return false;
        }
        ref = (ChunkRef*)base;
        q = (PointQuery*)((uint8_t*)base + 256);
        out = (int64_t*)((uint8_t*)base + 256 + kPoints * sizeof(PointQuery));
        return true;
    }
    // (never freed: a thread_local destructor of the main thread would run after the HIP runtime has shut down; one page per
    // host thread that ever asked a single point lives as long as the process)
};
thread_local PinnedPage g_page;
}  // namespace

static int run_points(const dcdf_chunk* h, const std::vector<PointQuery>& pq, int64_t* out) {
    const uint32_t n = (uint32_t)pq.size();
    if (n <= PinnedPage::kPoints && g_page.init()) {
        *g_page.ref = make_ref(h);
        std::memcpy(g_page.q, pq.data(), n * sizeof(PointQuery));
        hipLaunchKernelGGL(k_get, dim3((n + 255) / 256), dim3(256), 0, 0, g_page.ref, g_page.q, n, g_page.out);
        K2R_HIP(hipGetLastError());
        K2R_HIP(hipStreamSynchronize(0));
        std::memcpy(out, g_page.out, n * 8ull);
        return DCDF_OK;
    }
    const ChunkRef ref = make_ref(h);
    DevBuf d_ref, d_q, d_o;
    K2R_HIP(upload(d_ref, &ref, sizeof(ref)));
    K2R_HIP(upload(d_q, pq));
    K2R_HIP(d_o.alloc(pq.size() * 8));
    hipLaunchKernelGGL(k_get, dim3((n + 255) / 256), dim3(256), 0, 0, d_ref.as<ChunkRef>(), d_q.as<PointQuery>(), n,
                       d_o.as<int64_t>());
    K2R_HIP(hipGetLastError());
    K2R_HIP(hipMemcpy(out, d_o.p, pq.size() * 8, hipMemcpyDeviceToHost));
    return DCDF_OK;
}
extern "C" int dcdf_chunk_get(const dcdf_chunk* h, uint32_t instant, uint32_t row, uint32_t col, int64_t* out) {
    if (!h || !out) return DCDF_ERR_BAD_ARG;
    if (instant >= h->instants || row >= h->rows || col >= h->cols) return DCDF_ERR_BOUNDS;
    std::vector<PointQuery> pq{PointQuery{0, instant, row, col}};
    return run_points(h, pq, out);
}
extern "C" int dcdf_chunk_fill_cell(const dcdf_chunk* h, uint32_t start, uint32_t end, uint32_t row, uint32_t col,
                                    int64_t* out) {
    if (!h || !out) return DCDF_ERR_BAD_ARG;
    if (start > end) std::swap(start, end);
    if (end > h->instants || row >= h->rows || col >= h->cols) return DCDF_ERR_BOUNDS;
    if (end == start) return DCDF_OK;
    std::vector<PointQuery> pq;
    for (uint32_t i = start; i < end; i++) pq.push_back(PointQuery{0, i, row, col});
    return run_points(h, pq, out);
}

// ---- batched machinery shared by the point, window and search batches ------------------------------
static int upload_refs(const std::vector<const dcdf_chunk*>& uniq, DevBuf& d_refs) {
    std::vector<ChunkRef> refs(uniq.size());
    for (size_t i = 0; i < uniq.size(); i++) refs[i] = make_ref(uniq[i]);
    K2R_HIP(upload(d_refs, refs));
    return DCDF_OK;
}
static void dedup_chunks(dcdf_chunk* const* chunks, size_t nq, std::vector<uint32_t>& idx,
                         std::vector<const dcdf_chunk*>& uniq) {
    // queries usually hit few distinct chunks repeatedly; map pointer -> dense index (sorted unique)
    std::vector<const dcdf_chunk*> sorted(chunks, chunks + nq);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    uniq = sorted;
    idx.resize(nq);
    for (size_t q = 0; q < nq; q++)
        idx[q] = (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), (const dcdf_chunk*)chunks[q]) - uniq.begin());
}

// many (chunk, point) pairs -- or (chunk, cell series) -- in ONE launch (Superchunk::get / fill_cell route many points,
// superchunk.rs:313-400); at[] = output position of each point, or null for "in order"
static int run_points_multi(dcdf_chunk* const* chunks, size_t nchunks_q, const std::vector<uint32_t>& chunk_of_point,
                            std::vector<PointQuery>& pq, const std::vector<uint64_t>* at, uint64_t out_elems, int64_t* out, int out_mem,
                            float* kernel_ms) {
    std::vector<uint32_t> cidx;
    std::vector<const dcdf_chunk*> uniq;
    dedup_chunks(chunks, nchunks_q, cidx, uniq);
    for (size_t i = 0; i < pq.size(); i++) pq[i].chunk = cidx[chunk_of_point[i]];
    DevBuf d_refs, d_q, d_at, d_o;
    int rc = upload_refs(uniq, d_refs);
    if (rc != DCDF_OK) return rc;
    const uint32_t n = (uint32_t)pq.size();
    K2R_HIP(upload(d_q, pq));
    int64_t* dst = out;
    if (out_mem == DCDF_MEM_HOST) {
        K2R_HIP(d_o.alloc(out_elems * 8));
        dst = d_o.as<int64_t>();
    }
    if (at) K2R_HIP(upload(d_at, *at));
    EventPair ev;
    K2R_HIP(ev.create());
    K2R_HIP(hipEventRecord(ev.e0, 0));
    if (at) hipLaunchKernelGGL(k_get_at, dim3((n + 255) / 256), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_q.as<PointQuery>(), n, dst, d_at.as<uint64_t>());
    else hipLaunchKernelGGL(k_get, dim3((n + 255) / 256), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_q.as<PointQuery>(), n, dst);
    K2R_HIP(hipEventRecord(ev.e1, 0));
    K2R_HIP(hipGetLastError());
    if (out_mem == DCDF_MEM_HOST) K2R_HIP(hipMemcpy(out, d_o.p, out_elems * 8, hipMemcpyDeviceToHost));
    else K2R_HIP(hipDeviceSynchronize());
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
extern "C" int dcdf_query_get_batch(dcdf_chunk* const* chunks, const uint32_t* points, size_t n, int64_t* out, int out_mem,
                                    float* kernel_ms) {
    if (!chunks || !points || !out || n == 0 || n > 0x7fffffffu || (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    std::vector<PointQuery> pq(n);
    std::vector<uint32_t> cop(n);
    for (size_t i = 0; i < n; i++) {
        const dcdf_chunk* h = chunks[i];
        if (!h) return DCDF_ERR_BAD_ARG;
        const uint32_t t = points[3 * i], r = points[3 * i + 1], c = points[3 * i + 2];
        if (t >= h->instants || r >= h->rows || c >= h->cols) return DCDF_ERR_BOUNDS;
        pq[i] = PointQuery{0, t, r, c};
        cop[i] = (uint32_t)i;
    }
    return run_points_multi(chunks, n, cop, pq, nullptr, n, out, out_mem, kernel_ms);
}
extern "C" int dcdf_query_fill_cell_batch(dcdf_chunk* const* chunks, const uint32_t* cells, size_t n, int64_t* out,
                                          const uint64_t* out_offset, int out_mem, float* kernel_ms) {
    if (!chunks || !cells || !out || !out_offset || n == 0 || n > 0x7fffffffu || (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    std::vector<PointQuery> pq;
    std::vector<uint32_t> cop;
    std::vector<uint64_t> at;
    uint64_t hi = 0;  // elements of a device `out` the series reach
    for (size_t i = 0; i < n; i++) {
        const dcdf_chunk* h = chunks[i];
        if (!h) return DCDF_ERR_BAD_ARG;
        uint32_t a = cells[4 * i], b = cells[4 * i + 1];
        const uint32_t r = cells[4 * i + 2], c = cells[4 * i + 3];
        if (a > b) std::swap(a, b);
        if (b > h->instants || r >= h->rows || c >= h->cols) return DCDF_ERR_BOUNDS;
        for (uint32_t t = a; t < b; t++) {
            pq.push_back(PointQuery{0, t, r, c});
            cop.push_back((uint32_t)i);
            at.push_back(out_offset[i] + (t - a));
        }
        hi = std::max<uint64_t>(hi, out_offset[i] + (b - a));
    }
    if (pq.empty()) return DCDF_OK;
    if (pq.size() > 0x7fffffffu) return DCDF_ERR_CAPACITY;
    if (out_mem == DCDF_MEM_HOST) {  // dense staging on the device, then scattered into the caller's array
        std::vector<uint64_t> dense(pq.size());
        for (size_t i = 0; i < dense.size(); i++) dense[i] = i;
        std::vector<int64_t> tmp(pq.size());
        const int rc = run_points_multi(chunks, n, cop, pq, nullptr, pq.size(), tmp.data(), DCDF_MEM_HOST, kernel_ms);
        if (rc != DCDF_OK) return rc;
        for (size_t i = 0; i < tmp.size(); i++) out[at[i]] = tmp[i];
        return DCDF_OK;
    }
    return run_points_multi(chunks, n, cop, pq, &at, hi, out, DCDF_MEM_DEVICE, kernel_ms);
}

// ---- wave items and their launchers (k2r_query_host.h) -----------------------------------------------------------------
int k2r::launch_window_items_dev(const DevBuf& d_refs, const WinItem* d_items, uint32_t n, void* d_out, int32_t dtype, hipEvent_t e0, hipEvent_t e1,
                                 bool node_wise, bool narrow) {
    const uint32_t grid = std::min<uint32_t>((n + 3) / 4, 256u * 16u);
    if (e0) K2R_HIP(hipEventRecord(e0, 0));
    if (node_wise) {
        if (dtype == DCDF_I64 && narrow) hipLaunchKernelGGL((k_window_wave2<4, true, false, int32_t>), dim3(grid), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_items, n, d_out, dtype);
        else if (dtype == DCDF_I64) hipLaunchKernelGGL((k_window_wave2<3, true>), dim3(grid), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_items, n, d_out, dtype);
        else if (narrow) hipLaunchKernelGGL((k_window_wave2<4, false, false, int32_t>), dim3(grid), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_items, n, d_out, dtype);
        else hipLaunchKernelGGL((k_window_wave2<3, false>), dim3(grid), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_items, n, d_out, dtype);
    }
    else hipLaunchKernelGGL(k_window_wave, dim3(grid), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_items, n, d_out, dtype);
    if (e1) K2R_HIP(hipEventRecord(e1, 0));
    K2R_HIP(hipGetLastError());
    K2R_HIP(hipDeviceSynchronize());
    return DCDF_OK;
}
static int launch_window_items(const DevBuf& d_refs, const std::vector<WinItem>& items, void* d_out, int32_t dtype, hipEvent_t e0, hipEvent_t e1,
                               bool node_wise, bool narrow) {
    DevBuf d_items;
    K2R_HIP(upload(d_items, items));
    return launch_window_items_dev(d_refs, d_items.as<WinItem>(), (uint32_t)items.size(), d_out, dtype, e0, e1, node_wise, narrow);
}
// the four SEARCH forms of the node-wise walk: 32- or 64-bit values, integer or value search
int k2r::launch_search_walk(const ChunkRef* d_refs, const WinItem* d_witems, uint32_t nw, void* d_wbits, const SearchExtra* d_sx, bool narrow,
                            bool value) {
    const dim3 grid(std::min<uint32_t>((nw + 3) / 4, 256u * 16u)), block(256);
    if (narrow && value)
        hipLaunchKernelGGL((k_window_wave2<4, false, true, int32_t, true, true>), grid, block, 0, 0, d_refs, d_witems, nw, d_wbits, (int32_t)DCDF_I64, d_sx);
    else if (value)
        hipLaunchKernelGGL((k_window_wave2<3, false, true, int64_t, true, true>), grid, block, 0, 0, d_refs, d_witems, nw, d_wbits, (int32_t)DCDF_I64, d_sx);
    else if (narrow)
        hipLaunchKernelGGL((k_window_wave2<4, false, true, int32_t>), grid, block, 0, 0, d_refs, d_witems, nw, d_wbits, (int32_t)DCDF_I64, d_sx);
    else
        hipLaunchKernelGGL((k_window_wave2<3, false, true>), grid, block, 0, 0, d_refs, d_witems, nw, d_wbits, (int32_t)DCDF_I64, d_sx);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}
int k2r::launch_search_count(const uint32_t* d_wbits, const SearchItem* d_items, const WinQuery* d_qs, uint32_t ni, uint32_t* d_counts) {
    hipLaunchKernelGGL(k_search_count, dim3((ni + 63) / 64), dim3(64), 0, 0, d_wbits, d_items, d_qs, ni, d_counts);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}
int k2r::launch_search_emit(const WinQuery* d_qs, const SearchItem* d_items, uint32_t ni, const uint32_t* d_bits, const uint32_t* d_wbits,
                            const uint64_t* d_offs, uint32_t* d_out) {
    hipLaunchKernelGGL(k_search_emit, dim3((ni + 63) / 64), dim3(64), 0, 0, d_qs, d_items, ni, d_bits, d_wbits, d_offs, d_out);
    K2R_HIP(hipGetLastError());
    return DCDF_OK;
}

// ---- windows ----------------------------------------------------------------------------------------------
extern "C" int dcdf_chunk_fill_window(const dcdf_chunk* h, const dcdf_cube* cube, void* out, int32_t out_dtype,
                                      int64_t stride_t, int64_t stride_r, int64_t stride_c) {
    if (!h || !cube || !out) return DCDF_ERR_BAD_ARG;
    if (!out_args_ok(out_dtype, DCDF_MEM_HOST)) return DCDF_ERR_BAD_ARG;
    const dcdf_cube c = norm_cube(*cube);
    if (!cube_in(h, c)) return DCDF_ERR_BOUNDS;
    const uint64_t wt = c.end - c.start, wr = c.bottom - c.top, wc = c.right - c.left;
    if (wt * wr * wc == 0) return DCDF_OK;
    const size_t es = elem_size(out_dtype);
    // decode into a dense device array of the requested type, then scatter into the caller's strides
    DevBuf d_ref, d_q, d_o;
    const ChunkRef ref = make_ref(h);
    WinQuery q{};
    q.chunk = 0; q.start = c.start; q.end = c.end; q.top = c.top; q.bottom = c.bottom; q.left = c.left; q.right = c.right;
    K2R_HIP(upload(d_ref, &ref, sizeof(ref)));
    K2R_HIP(upload(d_q, &q, sizeof(q)));
    K2R_HIP(d_o.alloc(wt * wr * wc * es));
    if (wave_kernel_ok(h)) {
        std::vector<WinItem> items;
        window_items(0, c, 0, items, node_kernel_ok(h));
        const int rc = launch_window_items(d_ref, items, d_o.p, out_dtype, nullptr, nullptr, node_kernel_ok(h), h->narrow32);
        if (rc != DCDF_OK) return rc;
    } else {
        hipLaunchKernelGGL(k_fill_window, dim3(1), dim3(256), 0, 0, d_ref.as<ChunkRef>(), d_q.as<WinQuery>(), 1u, d_o.p,
                           out_dtype, (int64_t)(wr * wc), (int64_t)wc, (int64_t)1, 1);
        K2R_HIP(hipGetLastError());
    }
    std::vector<uint8_t> dense(wt * wr * wc * es);
    K2R_HIP(hipMemcpy(dense.data(), d_o.p, dense.size(), hipMemcpyDeviceToHost));
    const bool contiguous = stride_c == 1 && stride_r == (int64_t)wc && stride_t == (int64_t)(wr * wc);
    if (contiguous) {
        std::memcpy(out, dense.data(), dense.size());
    } else {
        const uint8_t* s = dense.data();
        for (uint64_t t = 0; t < wt; t++)
            for (uint64_t r = 0; r < wr; r++)
                for (uint64_t cc = 0; cc < wc; cc++, s += es)
                    std::memcpy((uint8_t*)out + ((int64_t)t * stride_t + (int64_t)r * stride_r + (int64_t)cc * stride_c) * (int64_t)es, s, es);
    }
    return DCDF_OK;
}

int k2r::search_impl(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper, size_t nq, uint32_t* out,
                     size_t cap, uint64_t* counts, uint64_t* offsets, size_t* total_out, float* kernel_ms, int out_mem, const SearchCtx* ctx,
                     const double* vlower, const double* vupper) {
    const bool value = vlower != nullptr;
    std::vector<uint32_t> cidx;
    std::vector<const dcdf_chunk*> uniq;
    if (!ctx) dedup_chunks(chunks, nq, cidx, uniq);
    std::vector<WinQuery> qs(nq);
    std::vector<SearchItem> items;
    // k = 2 chunks: the wave-cooperative walk of fill_window marks the matches (one wave per piece of <= 64 x 64 cells and
    // instant, each into its own 128-word bitmap; the instants of dcdf_chunk::search_quirk carry a flag); other arities are
    // decoded and tested cell by cell (k_search_cells) into a flat per-item bitmap
    bool node_wise = std::getenv("K2R_SEARCH_DFS") == nullptr;  // (diagnostics: A/B against the cell-by-cell kernel)
    for (const dcdf_chunk* u : uniq) node_wise = node_wise && node_kernel_ok(u);
    if (ctx) node_wise = node_wise && ctx->node_wise;
    // other arities with k * k <= 64: the pruned wave walk k_search_wave, one wave per (item, sub-window of <= 32 x 32 cells), into the
    // item's flat window bitmap; what is left (k > 8) is decoded and tested cell by cell
    bool wave_search = !node_wise && std::getenv("K2R_SEARCH_CELLS") == nullptr;
    for (const dcdf_chunk* u : uniq) wave_search = wave_search && wave_kernel_ok(u);
    if (ctx) wave_search = wave_search && ctx->wave_ok;
    std::vector<WinItem> witems;
    std::vector<SearchExtra> sx;
    std::vector<uint8_t> item_quirk;  // per item of the decode-and-test kernel
    uint64_t bits_words = 0;
    size_t n_dfs = 0;
    for (size_t q = 0; q < nq; q++) {
        if (!chunks[q]) return DCDF_ERR_BAD_ARG;
        const dcdf_cube c = norm_cube(cubes[q]);
        if (!cube_in(chunks[q], c)) return DCDF_ERR_BOUNDS;
        WinQuery& Q = qs[q];
        Q = WinQuery{};
        Q.chunk = ctx ? ctx->chunk_of[q] : cidx[q];
        if (ctx) {
            Q._pad = ctx->origin[3 * q];
            Q.out_off = (uint64_t)ctx->origin[3 * q + 1] | (uint64_t)ctx->origin[3 * q + 2] << 32;
        }
        Q.start = c.start; Q.end = c.end; Q.top = c.top; Q.bottom = c.bottom; Q.left = c.left; Q.right = c.right;
        bool hole = false;
        if (value) {
            ValueRange vr;
            if (!value_bounds(chunks[q]->encoding, chunks[q]->fbits, vlower[q], vupper[q], &vr)) return DCDF_ERR_BAD_ARG;
            // a narrow chunk's values all lie in [-2^30, 2^30): its walk needs no more than the int32 part of the range
            if (!vr.empty && chunks[q]->narrow32) {
                vr.lo = std::max<int64_t>(vr.lo, INT32_MIN);
                vr.hi = std::min<int64_t>(vr.hi, INT32_MAX);
                vr.empty = vr.lo > vr.hi;
            }
            Q.lower = vr.lo;
            Q.upper = vr.hi;
            hole = vr.hole;
            if (vr.empty) continue;  // no items: nothing can match
        } else {
            Q.lower = std::min(lower[q], upper[q]);  // helpers.rs:7-16 via chunk.rs:214
            Q.upper = std::max(lower[q], upper[q]);
        }
        // the per-item flag of the walks: the reference quirk of the instant, or (value search) the hole
        auto flag = [&](uint32_t i) -> uint8_t { return value ? (hole ? 1 : 0) : chunks[q]->search_quirk[i]; };
        const uint64_t cells = (uint64_t)(c.bottom - c.top) * (c.right - c.left);
        if (cells == 0) continue;
        const uint32_t ncb = (c.right - c.left + 63u) >> 6;
        for (uint32_t i = c.start; i < c.end; i++) {
            if (node_wise) {
                if (witems.size() + 4096 > 0xffffff00u) return DCDF_ERR_CAPACITY;
                items.push_back(SearchItem{(uint32_t)q, i, 0, (uint32_t)witems.size(), ncb});
                for (uint32_t r = c.top; r < c.bottom; r += 64)
                    for (uint32_t cc = c.left; cc < c.right; cc += 64) {
                        WinItem it{};
                        it.chunk = Q.chunk;
                        it.inst = i;
                        it.top = (uint16_t)r;
                        it.bottom = (uint16_t)std::min(r + 64, c.bottom);
                        it.left = (uint16_t)cc;
                        it.right = (uint16_t)std::min(cc + 64, c.right);
                        witems.push_back(it);
                        sx.push_back(SearchExtra{Q.lower, Q.upper, flag(i) ? 1u : 0u, 0u});
                    }
            } else {
                items.push_back(SearchItem{(uint32_t)q, i, bits_words, SI_FLAT, 0});
                item_quirk.resize(items.size(), 0);
                item_quirk.back() = flag(i);
                if (wave_search) {
                    if (witems.size() + 4096 > 0xffffff00u) return DCDF_ERR_CAPACITY;
                    // bit (r, c) of the item's flat bitmap = out_off + (r - top) * out_sr + (c - left): the window's own dense layout
                    window_items(Q.chunk, dcdf_cube{i, i + 1, c.top, c.bottom, c.left, c.right}, bits_words * 32ull, witems, false);
                    sx.resize(witems.size(), SearchExtra{Q.lower, Q.upper, flag(i) ? 1u : 0u, (uint32_t)(items.size() - 1)});
                }
                bits_words += (cells + 31) / 32;
                n_dfs++;
            }
        }
    }
    for (size_t q = 0; q < nq; q++) counts[q] = 0;
    float ms_total = 0.f;
    std::vector<uint32_t> item_counts(items.size());
    DevBuf d_refs_own, d_qs, d_items, d_bits, d_wbits, d_witems, d_sx, d_counts, d_offs, d_out, d_quirk;
    if (!items.empty()) {
        if (!ctx) {
            int rc = upload_refs(uniq, d_refs_own);
            if (rc != DCDF_OK) return rc;
        }
        const DevBuf& d_refs = ctx ? *ctx->refs : d_refs_own;
        K2R_HIP(upload(d_qs, qs));
        K2R_HIP(upload(d_items, items));
        if (n_dfs) {
            K2R_HIP(d_bits.alloc(std::max<uint64_t>(bits_words, 1) * 4));
            K2R_HIP(hipMemset(d_bits.p, 0, std::max<uint64_t>(bits_words, 1) * 4));
        }
        const uint32_t nw = (uint32_t)witems.size();
        if (nw) {
            K2R_HIP(upload(d_witems, witems));
            K2R_HIP(upload(d_sx, sx));
            if (node_wise) K2R_HIP(d_wbits.alloc((size_t)nw * 512));  // (every word is written by the walk: nothing to clear)
        }
        K2R_HIP(d_counts.alloc(items.size() * 4));
        if (wave_search) K2R_HIP(hipMemset(d_counts.p, 0, items.size() * 4));  // (several waves add to an item's count)
        EventPair ev;
        K2R_HIP(ev.create());
        const hipEvent_t e0 = ev.e0, e1 = ev.e1;
        const uint32_t ni = (uint32_t)items.size();
        K2R_HIP(hipEventRecord(e0, 0));
        const uint32_t gw = std::min<uint32_t>((nw + 3) / 4, 256u * 16u);
        if (nw && wave_search) {
            if (value)
                hipLaunchKernelGGL(k_search_wave<true>, dim3(gw), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_witems.as<WinItem>(), nw,
                                   d_sx.as<SearchExtra>(), d_bits.as<uint32_t>(), d_counts.as<uint32_t>());
            else
                hipLaunchKernelGGL(k_search_wave<false>, dim3(gw), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_witems.as<WinItem>(), nw,
                                   d_sx.as<SearchExtra>(), d_bits.as<uint32_t>(), d_counts.as<uint32_t>());
        } else if (nw) {
            bool all_narrow = true;
            for (const dcdf_chunk* u : uniq) all_narrow = all_narrow && u->narrow32;
            if (ctx) all_narrow = ctx->all_narrow;
            int rc = launch_search_walk(d_refs.as<ChunkRef>(), d_witems.as<WinItem>(), nw, d_wbits.p, d_sx.as<SearchExtra>(), all_narrow, value);
            if (rc == DCDF_OK) rc = launch_search_count(d_wbits.as<uint32_t>(), d_items.as<SearchItem>(), d_qs.as<WinQuery>(), ni, d_counts.as<uint32_t>());
            if (rc != DCDF_OK) return rc;
        }
        if (n_dfs && !wave_search) {
            item_quirk.resize(items.size(), 0);
            K2R_HIP(upload(d_quirk, item_quirk));
            if (value)
                hipLaunchKernelGGL(k_search_cells<true>, dim3(ni), dim3(64), 0, 0, d_refs.as<ChunkRef>(), d_qs.as<WinQuery>(),
                                   d_items.as<SearchItem>(), ni, d_quirk.as<uint8_t>(), d_bits.as<uint32_t>(), d_counts.as<uint32_t>());
            else
                hipLaunchKernelGGL(k_search_cells<false>, dim3(ni), dim3(64), 0, 0, d_refs.as<ChunkRef>(), d_qs.as<WinQuery>(),
                                   d_items.as<SearchItem>(), ni, d_quirk.as<uint8_t>(), d_bits.as<uint32_t>(), d_counts.as<uint32_t>());
        }
        K2R_HIP(hipEventRecord(e1, 0));
        K2R_HIP(hipGetLastError());
        K2R_HIP(hipMemcpy(item_counts.data(), d_counts.p, items.size() * 4, hipMemcpyDeviceToHost));
        float ms = 0.f;
        K2R_HIP(hipEventElapsedTime(&ms, e0, e1));
        ms_total += ms;
        std::vector<uint64_t> item_offs(items.size());
        uint64_t run = 0;
        for (size_t i = 0; i < items.size(); i++) {
            item_offs[i] = run;
            run += item_counts[i];
            counts[items[i].query] += item_counts[i];
        }
        *total_out = run;
        uint64_t acc = 0;
        for (size_t q = 0; q < nq; q++) {
            offsets[q] = acc;
            acc += counts[q];
        }
        if (run > cap) return DCDF_ERR_CAPACITY;
        if (run > 0) {
            K2R_HIP(upload(d_offs, item_offs));
            const bool to_dev = out_mem == DCDF_MEM_DEVICE;  // the triples stay where the emit kernel writes them
            if (!to_dev) K2R_HIP(d_out.alloc(run * 12));
            K2R_HIP(hipEventRecord(e0, 0));
            const int rc = launch_search_emit(d_qs.as<WinQuery>(), d_items.as<SearchItem>(), ni, d_bits.as<uint32_t>(), d_wbits.as<uint32_t>(),
                                              d_offs.as<uint64_t>(), to_dev ? out : d_out.as<uint32_t>());
            K2R_HIP(hipEventRecord(e1, 0));
            if (rc != DCDF_OK) return rc;
            if (to_dev) K2R_HIP(hipDeviceSynchronize());
            else K2R_HIP(hipMemcpy(out, d_out.p, run * 12, hipMemcpyDeviceToHost));
            K2R_HIP(hipEventElapsedTime(&ms, e0, e1));
            ms_total += ms;
        }
    } else {
        *total_out = 0;
        for (size_t q = 0; q < nq; q++) offsets[q] = 0;
    }
    if (kernel_ms) *kernel_ms = ms_total;
    return DCDF_OK;
}

extern "C" int dcdf_chunk_search(const dcdf_chunk* h, const dcdf_cube* cube, int64_t lower, int64_t upper,
                                 uint32_t* out, size_t cap, size_t* n) {
    if (!h || !cube || !n || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    dcdf_chunk* hp = const_cast<dcdf_chunk*>(h);
    uint64_t cnt = 0, off = 0;
    size_t total = 0;
    const int rc = search_impl(&hp, cube, &lower, &upper, 1, out, cap, &cnt, &off, &total, nullptr);
    *n = total;
    return rc;
}

// value search (real-valued bounds, translated per chunk by value_bounds on the host; see dcdf_k2r.h)
extern "C" int dcdf_chunk_search_values(const dcdf_chunk* h, const dcdf_cube* cube, double lower, double upper, uint32_t* out, size_t cap,
                                        size_t* n) {
    if (!h || !cube || !n || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (lower != lower || upper != upper) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    dcdf_chunk* hp = const_cast<dcdf_chunk*>(h);
    uint64_t cnt = 0, off = 0;
    size_t total = 0;
    const int rc = search_impl(&hp, cube, nullptr, nullptr, 1, out, cap, &cnt, &off, &total, nullptr, DCDF_MEM_HOST, nullptr, &lower, &upper);
    *n = total;
    return rc;
}
extern "C" int dcdf_value_bounds(int32_t encoding, uint32_t fractional_bits, double lower, double upper, int64_t* lo, int64_t* hi,
                                 int32_t* skip_zero) {
    if (!lo || !hi || !skip_zero) return DCDF_ERR_BAD_ARG;
    ValueRange vr;
    if (!value_bounds(encoding, fractional_bits, lower, upper, &vr)) return DCDF_ERR_BAD_ARG;
    *lo = vr.lo;
    *hi = vr.hi;
    *skip_zero = vr.hole ? 1 : 0;
    return DCDF_OK;
}

extern "C" int dcdf_query_search_batch(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const int64_t* lower,
                                       const int64_t* upper, size_t nq, uint32_t* out, size_t cap, uint64_t* counts,
                                       uint64_t* offsets, float* kernel_ms) {
    if (!chunks || !cubes || !lower || !upper || !counts || !offsets || nq == 0 || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    size_t total = 0;
    return search_impl(chunks, cubes, lower, upper, nq, out, cap, counts, offsets, &total, kernel_ms);
}

// out_dtype: the element type written (MMBuffer3::set conversion of the stored value, mmbuffer.rs:292-299: i32 / i64 as is,
// f32 / f64 through from_fixed); out_mem: `out` is host or DEVICE memory -- a device `out` is written by the decode kernel
// itself at out_offset[q] (elements), nothing crosses PCIe
static int fill_window_batch_impl(dcdf_chunk* const* chunks, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype, int out_mem,
                                  const uint64_t* out_offset, float* kernel_ms) {
    if (!chunks || !cubes || !out || !out_offset || nq == 0) return DCDF_ERR_BAD_ARG;
    if (!out_args_ok(out_dtype, out_mem)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    std::vector<uint32_t> cidx;
    std::vector<const dcdf_chunk*> uniq;
    dedup_chunks(chunks, nq, cidx, uniq);
    std::vector<WinQuery> qs(nq);
    WindowOut W(cubes, nq, out, out_offset, elem_size(out_dtype), out_mem == DCDF_MEM_DEVICE);
    for (size_t q = 0; q < nq; q++) {
        if (!chunks[q]) return DCDF_ERR_BAD_ARG;
        const dcdf_cube c = norm_cube(cubes[q]);
        if (!cube_in(chunks[q], c)) return DCDF_ERR_BOUNDS;
        WinQuery& Q = qs[q];
        Q = WinQuery{};
        Q.chunk = cidx[q];
        Q.start = c.start; Q.end = c.end; Q.top = c.top; Q.bottom = c.bottom; Q.left = c.left; Q.right = c.right;
        Q.out_off = W.base[q];
    }
    if (W.total == 0) return DCDF_OK;
    DevBuf d_refs, d_qs;
    int rc = upload_refs(uniq, d_refs);
    if (rc != DCDF_OK) return rc;
    K2R_HIP(upload(d_qs, qs));
    if (!W.to_dev) K2R_HIP(W.stage.alloc(W.total * W.es));
    void* const d_dst = W.dst();
    EventPair ev;
    K2R_HIP(ev.create());
    bool all_wave = true, all_node = true;
    bool all_narrow = true;
    for (const dcdf_chunk* u : uniq) {
        all_wave = all_wave && wave_kernel_ok(u);
        all_node = all_node && node_kernel_ok(u);
        all_narrow = all_narrow && u->narrow32;
    }
    if (all_wave) {
        std::vector<WinItem> items;
        for (size_t q = 0; q < nq; q++) {
            const dcdf_cube c{qs[q].start, qs[q].end, qs[q].top, qs[q].bottom, qs[q].left, qs[q].right};
            window_items(qs[q].chunk, c, qs[q].out_off, items, all_node);
        }
        rc = launch_window_items(d_refs, items, d_dst, out_dtype, ev.e0, ev.e1, all_node, all_narrow);
        if (rc != DCDF_OK) return rc;
    } else {
        // arities beyond the wave walk (k * k > 64): per-cell descents, typed at each query's out_off like the walks
        const uint32_t grid = (uint32_t)std::min<size_t>(nq, 1u << 20);
        K2R_HIP(hipEventRecord(ev.e0, 0));
        hipLaunchKernelGGL(k_fill_window, dim3(grid), dim3(256), 0, 0, d_refs.as<ChunkRef>(), d_qs.as<WinQuery>(),
                           (uint32_t)nq, d_dst, out_dtype, (int64_t)0, (int64_t)0, (int64_t)0, 0);
        K2R_HIP(hipEventRecord(ev.e1, 0));
        K2R_HIP(hipGetLastError());
        K2R_HIP(hipDeviceSynchronize());
    }
    rc = W.finish();
    if (rc != DCDF_OK) return rc;
    float ms = 0.f;
    K2R_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = ms;
    return DCDF_OK;
}
extern "C" int dcdf_query_search_batch_mem(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const int64_t* lower,
                                           const int64_t* upper, size_t nq, uint32_t* out, size_t cap, int out_mem,
                                           uint64_t* counts, uint64_t* offsets, float* kernel_ms) {
    if (!chunks || !cubes || !lower || !upper || !counts || !offsets || nq == 0 || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    size_t total = 0;
    return search_impl(chunks, cubes, lower, upper, nq, out, cap, counts, offsets, &total, kernel_ms, out_mem);
}
extern "C" int dcdf_query_search_values_batch(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const double* lower, const double* upper,
                                              size_t nq, uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets,
                                              float* kernel_ms) {
    if (!chunks || !cubes || !lower || !upper || !counts || !offsets || nq == 0 || (!out && cap)) return DCDF_ERR_BAD_ARG;
    if (out_mem != DCDF_MEM_HOST && out_mem != DCDF_MEM_DEVICE) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    size_t total = 0;
    return search_impl(chunks, cubes, nullptr, nullptr, nq, out, cap, counts, offsets, &total, kernel_ms, out_mem, nullptr, lower, upper);
}
extern "C" int dcdf_query_fill_window_batch(dcdf_chunk* const* chunks, const dcdf_cube* cubes, size_t nq, int64_t* out,
                                            const uint64_t* out_offset, float* kernel_ms) {
    return fill_window_batch_impl(chunks, cubes, nq, out, (int32_t)DCDF_I64, DCDF_MEM_HOST, out_offset, kernel_ms);
}
extern "C" int dcdf_query_fill_window_batch_typed(dcdf_chunk* const* chunks, const dcdf_cube* cubes, size_t nq, void* out,
                                                  int32_t out_dtype, int out_mem, const uint64_t* out_offset, float* kernel_ms) {
    return fill_window_batch_impl(chunks, cubes, nq, out, out_dtype, out_mem, out_offset, kernel_ms);
}
