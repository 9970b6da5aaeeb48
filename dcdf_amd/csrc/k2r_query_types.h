// k2r_query_types.h -- what the query-side translation units share: the device-visible chunk handle with its side-16
// tables, and the k = 2 node-wise readers of the serialized streams (four adjacent children per lane).
#pragma once
#include <type_traits>

#include "k2r_decode.h"
#include "k2r_items.h"

namespace k2r {

struct TopEnt {  // the walk's state at one node (log.rs:360-361): both first-child indices NONE = its square has the one value mt + ms
    uint32_t bt, bs;
    int32_t mt, ms;  // (a chunk with a value beyond int32 gets no table: k_top_table reports it)
};
struct TopMM {  // smallest and largest value inside the same square (the reference's own pruning bounds: log.rs:573-574)
    int32_t vmin, vmax;
};
struct ChunkRef {  // device-visible handle of an opened chunk
    const uint8_t* bytes;
    const InstDesc* descs;
    uint32_t instants, rows, cols, fbits;
    const TopEnt* top;  // [instant][top_g * top_g] or null
    const TopMM* top_mm;  // the same squares' value ranges (search prunes with them)
    uint32_t top_g, _pad;
};

constexpr uint32_t WQ_NONE = 0xffffffffu;
struct GpuExecScan {  // inclusive prefix sum over the 64 lanes (DPP), as GpuExec::wave_incl_scan
    __device__ __forceinline__ static uint32_t incl(uint32_t v) {
        int x = (int)v;
        x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);
        x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);
        x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);
        x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);
        x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
        x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
        return (uint32_t)x;
    }
};

// ---- k = 2, node-wise: one lane per frontier NODE, its four children share their loads ---------------------------------
// Siblings are adjacent in every stream (children of a node sit at base .. base + 3): their four T bits and ranks come from
// ONE 16-byte load of the rank block (+ its index word), their four Lmax bytes from ONE 4-byte load, their continuation bits
// from the same kind of block load, the second bytes of the long ones from one more 4-byte load.  ~14 loads per node for both
// trees instead of ~18 per CHILD.
struct Blk16 {
    uint32_t w[4];
} __attribute__((aligned(1)));
// The chunk bytes are global memory, but a pointer loaded from a table is "generic" to the compiler and every access through
// it a FLAT instruction (slower, and counted in both wait counters): the node-wise walk uses address-space-1 pointers.
typedef const __attribute__((address_space(1))) uint8_t* gbytes;
__device__ __forceinline__ uint32_t gld32(gbytes p) {  // unaligned 4-byte load, native order
    typedef uint32_t __attribute__((aligned(1))) u32u;
    return *(const __attribute__((address_space(1))) u32u*)p;
}
__device__ __forceinline__ uint32_t gld_be32(gbytes p) { return __builtin_bswap32(gld32(p)); }
__device__ __forceinline__ bool gbm_get(gbytes b, const BmDesc& d, uint32_t i) {
    const uint32_t w = i >> 5;
    if (w >= (d.len + 31) / 32) return false;
    return (gld_be32(b + d.words_off + 4 * w) >> (31 - (i & 31))) & 1u;
}
// rank1(T, i) and the four bits i .. i+3 (bit i = 8), bits at or beyond d.len read as 0.  Needs d.k == 4 and i < d.len.
__device__ __forceinline__ uint32_t rank_nib(gbytes b, const BmDesc& d, uint32_t i, uint32_t* nib) {
    const uint32_t w0 = i >> 5, blk = w0 >> 2, sh = i & 31u;
    uint32_t cnt = blk ? gld_be32(b + d.idx_off + 4 * (blk - 1)) : 0u;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(1)));
    const u32x4 raw = *(const __attribute__((address_space(1))) u32x4*)(b + d.words_off + 16 * blk);
    const uint32_t w[4] = {__builtin_bswap32(raw.x), __builtin_bswap32(raw.y), __builtin_bswap32(raw.z), __builtin_bswap32(raw.w)};
    const uint32_t q0 = w0 & 3u;
    uint32_t x = w[0], nx = w[1];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if ((uint32_t)q < q0) cnt += popc32(w[q]);
        if ((uint32_t)q == q0) {
            x = w[q];
            nx = q < 3 ? w[q + 1] : 0u;
        }
    }
    if (q0 == 3 && sh > 28) nx = gld_be32(b + d.words_off + 4 * (w0 + 1));  // the group of four straddles the block's end (3 in 128)
    if (sh) cnt += popc32(x >> (32 - sh));
    uint32_t n4 = (uint32_t)(((((uint64_t)x << 32) | nx) >> (60 - sh)) & 15u);
    const uint32_t valid = d.len - i;  // > 0
    if (valid < 4) n4 &= (0xfu << (4 - valid)) & 0xfu;
    *nib = n4;
    return cnt;
}
// What the node-wise walk needs of one tree, copied out of its InstDesc once per item (wave-uniform: lives in SGPRs instead
// of being re-fetched through a pointer the compiler must assume the output stores alias).
struct TreeRef {
    BmDesc T, E, c0, c1;      // T, eqB, continuation bitmaps of the Lmax Dac's planes 0 and 1
    uint32_t by0, by1, nlev;  // Lmax plane-0 / plane-1 bytes, number of planes
};
typedef const __attribute__((address_space(1))) InstDesc* gdesc;
__device__ __forceinline__ BmDesc bm_copy(const __attribute__((address_space(1))) BmDesc* p) { return BmDesc{p->len, p->k, p->idx_off, p->words_off}; }
__device__ __forceinline__ TreeRef tree_ref(gdesc p) {
    TreeRef t;
    t.T = bm_copy(&p->T); t.E = bm_copy(&p->E); t.c0 = bm_copy(&p->mx.bm[0]); t.c1 = bm_copy(&p->mx.bm[1]);
    t.by0 = p->mx.bytes_off[0]; t.by1 = p->mx.bytes_off[1]; t.nlev = p->mx.nlev;
    return t;
}
__device__ __forceinline__ TreeRef tree_ref(const InstDesc& d) {
    TreeRef t;
    t.T = d.T; t.E = d.E; t.c0 = d.mx.bm[0]; t.c1 = d.mx.bm[1];
    t.by0 = d.mx.bytes_off[0]; t.by1 = d.mx.bytes_off[1]; t.nlev = d.mx.nlev;
    return t;
}
// the four Lmax values at index i .. i+3 (those at or beyond the Dac's length: 0); `full` = the whole Dac, for values of
// three or more bytes (rare)
template <class V>
__device__ __forceinline__ void dac4(gbytes b, const TreeRef& t, const DacDesc& full, uint32_t i, V (&out)[4]) {
    typedef typename std::conditional<sizeof(V) == 4, uint32_t, uint64_t>::type U;
    const uint32_t len = t.c0.len;
    const uint32_t b0 = gld32(b + t.by0 + i);
    uint32_t cb = 0, r0 = 0;
    if (t.nlev > 1) r0 = rank_nib(b, t.c0, i, &cb);
    uint32_t cb1 = 0;
    const uint32_t b1 = gld32(b + t.by1 + r0);  // (no branch: with a single plane by1 = r0 = 0, a harmless read of the chunk's first bytes)
    if (t.nlev > 2 && cb) (void)rank_nib(b, t.c1, r0, &cb1);
    uint32_t q = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        U n = (b0 >> (8 * c)) & 0xffu;
        const bool more = (cb >> (3 - c)) & 1u;
        if (more) {
            if ((cb1 >> (3 - q)) & 1u) {  // three or more bytes: the general walk
                out[c] = i + c < len ? (V)dacd_get((const uint8_t*)b, full, i + c) : (V)0;
                q++;
                continue;
            }
            n |= (U)((b1 >> (8 * q)) & 0xffu) << 8;
            q++;
        }
        out[c] = i + c < len ? (V)((n >> 1) ^ ((U)0 - (n & 1))) : (V)0;
    }
}
// bits i .. i + 3 of a bitmap (bit i = 8), bits beyond its words read as 0 like gbm_get; two loads, no branch
__device__ __forceinline__ uint32_t gbm_get4(gbytes b, const BmDesc& d, uint32_t i) {
    const uint32_t nw = (d.len + 31) / 32, w = i >> 5, sh = i & 31u;
    const uint32_t w0 = w < nw ? w : 0u, w1 = w + 1 < nw ? w + 1 : 0u;
    uint32_t x = gld_be32(b + d.words_off + 4 * w0), y = gld_be32(b + d.words_off + 4 * w1);
    x = w < nw ? x : 0u;
    y = w + 1 < nw ? y : 0u;
    return (uint32_t)(((((uint64_t)x << 32) | y) >> (60 - sh)) & 15u);
}


// ---- what the kernels of more than one translation unit, and the host code that feeds them, read ------------------------------------
struct WinQuery {  // one fill_window / search request against one chunk
    uint32_t chunk;
    uint32_t start, end, top, bottom, left, right;
    uint32_t _pad;
    int64_t lower, upper;
    uint64_t out_off;  // fill_window: first output element
};
// one (query, instant) of a search: its window bitmap
struct SearchItem {
    uint32_t query, instant;  // instant is absolute within the chunk
    uint64_t bits_off;        // u32 words: the item's window bitmap, row-major over the query window (per-thread descent)
    uint32_t w0, ncb;         // wave walk: first of the item's pieces (<= 64 x 64 cells from the window's origin, row-major; a bitmap
                              // of 64 rows x 2 words each) and pieces per row; w0 == SI_FLAT: the flat bitmap above is the one in use
};
constexpr uint32_t SI_FLAT = 0xffffffffu;
struct SearchExtra {
    int64_t lower, upper;
    // The reference's Log::search_window has no case for a single-node UNIFORM log over a multi-node snapshot (log.rs:527-548):
    // it never reads eqB[0], seeds min_t with an empty Dac's 0 and descends the snapshot as if the log were "equal" with the
    // root's difference.  Read as data, its result for such an instant is: every cell when min_s(root) >= lower and c <= upper
    // (c = the instant's one value), no cell when min_s(root) > upper or c < lower, and otherwise the cells with
    // lower <= s(cell) + (c - max_s(root)) <= upper.  quirk != 0 makes the walk do exactly that instead of the decode of the
    // instant's true values.
    uint32_t quirk, _pad;
};
struct PointQuery {  // get / fill_cell: one cell
    uint32_t chunk, instant, row, col;
};
// counts of the (query, instant) items the wave walk marked: one thread each over the bitmaps of the item's pieces
__device__ __forceinline__ uint32_t search_count_wave_item(const uint32_t* __restrict__ wbits, const SearchItem& I, const WinQuery& Q) {
    const uint32_t nrb = (Q.bottom - Q.top + 63u) >> 6;
    const uint4* w = (const uint4*)(wbits + (uint64_t)I.w0 * 128u);
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < nrb * I.ncb * 32u; i++) {
        const uint4 x = w[i];
        cnt += popc32(x.x) + popc32(x.y) + popc32(x.z) + popc32(x.w);
    }
    return cnt;
}
// the triples of one wave-walk item: the pieces' bitmaps (64 rows x 2 words), rows in order, pieces left to right; the origin of
// the chunk inside its raster (dcdf_raster_search_batch; zero for chunk-level searches) is added: a search does not use out_off /
// _pad otherwise
__device__ __forceinline__ void search_emit_wave_item(const SearchItem& I, const WinQuery& Q, const uint32_t* __restrict__ wbits,
                                                      uint32_t* __restrict__ o) {
    const uint32_t ot = Q._pad, orow = (uint32_t)Q.out_off, ocol = (uint32_t)(Q.out_off >> 32);
    for (uint32_t r = Q.top; r < Q.bottom; r++) {
        const uint32_t rb = (r - Q.top) >> 6, rr = (r - Q.top) & 63u;
        for (uint32_t cw = 0; cw < 2u * I.ncb; cw++) {
            uint32_t x = wbits[((uint64_t)I.w0 + rb * I.ncb + (cw >> 1)) * 128u + 2u * rr + (cw & 1u)];
            while (x) {
                const uint32_t j = (uint32_t)__builtin_ctz(x);
                x &= x - 1;
                o[0] = ot + I.instant;
                o[1] = orow + r;
                o[2] = ocol + Q.left + 32u * cw + j;
                o += 3;
            }
        }
    }
}

// ---- the node-wise walk's state and its step: shared by the query walks (k2r_query.hip) and the side-16 tables (k2r_open.hip) -------
// V = int64_t in general; int32_t for chunks whose stored values all lie in [-2^30, 2^30) (dcdf_chunk::narrow32: every node
// extreme and every log difference then fits 32 bits), which halves the walk's arithmetic and its register footprint
template <class V>
struct NodeStT {
    uint32_t bt, bs;  // index of the node's FIRST CHILD in the log / snapshot tree (1 + rank(T, node) * k^2), or NONE
    V mt, ms;         // log.rs:360-361 max_t, max_s
};
typedef NodeStT<int64_t> NodeSt;
template <class V>
struct KidsT {
    NodeStT<V> st[4];
    V val[4];
    uint32_t fill;  // bit c: child c's whole square has the single value val[c]
};
typedef KidsT<int64_t> Kids;
// the four children of node p (log.rs:392-505 / snapshot.rs:281-299 for all of i, j at once)
template <class V>
__device__ __forceinline__ void expand4(gbytes b, const TreeRef& S, const DacDesc& Sfull, const TreeRef& L, const DacDesc& Lfull,
                                        const NodeStT<V>& p, KidsT<V>* o) {
    // Every read below is unconditional (a side that has nothing to read reads index 0 and drops the result): behind
    // `if (has_t)` / `if (has_s)` / per-child branches the log's chain of dependent loads, the snapshot's and up to four eqB
    // reads ran one after the other; this way they are in flight together.
    const bool has_t = p.bt != WQ_NONE, has_s = p.bs != WQ_NONE;
    const bool cells_t = !has_t || p.bt >= L.T.len, cells_s = !has_s || p.bs >= S.T.len;  // the children are beyond T: cells
    V dt[4], ds[4];
    dac4(b, L, Lfull, has_t ? p.bt : 0u, dt);
    dac4(b, S, Sfull, has_s ? p.bs : 0u, ds);
    uint32_t tt = 0, ts = 0;  // T nibbles (bit c = 8 >> c) and rank of the first child
    uint32_t rt = rank_nib(b, L.T, cells_t ? 0u : p.bt, &tt), rs = rank_nib(b, S.T, cells_s ? 0u : p.bs, &ts);
    if (cells_t) { tt = 0; rt = 0; }
    if (cells_s) { ts = 0; rs = 0; }
    // eqB bits of the children with T = 0 (log.rs:452-467): child c's is eqB[p.bt + c - rank(T, p.bt + c)] = the (zeros among the
    // children before c)-th bit from eqB[p.bt - rt] on -- four consecutive bits at most
    const uint32_t eq4 = gbm_get4(b, L.E, cells_t ? 0u : p.bt - rt);
    V vt[4], vs[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        vt[c] = has_t ? dt[c] : p.mt;
        vs[c] = has_s ? ds[c] : (V)0;
    }
    o->fill = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const bool bit_t = (tt >> (3 - c)) & 1u, bit_s = (ts >> (3 - c)) & 1u;
        const bool leaf_t = !has_t || cells_t || !bit_t, leaf_s = !has_s || cells_s || !bit_s;
        const uint32_t before_t = popc32(tt >> (4 - c));
        const uint32_t rtc = rt + before_t, rsc = rs + popc32(ts >> (4 - c));  // rank(T, base + c)
        const V mt_ = vt[c], ms_ = has_s ? p.ms - vs[c] : p.ms;
        o->val[c] = mt_ + ms_;
        NodeStT<V>& n = o->st[c];
        n.mt = mt_;
        n.ms = ms_;
        n.bt = WQ_NONE;
        n.bs = WQ_NONE;
        if (leaf_t && leaf_s) {
            o->fill |= 1u << c;
        } else if (leaf_s) {
            n.bt = 1 + rtc * 4;
        } else if (leaf_t) {
            const bool eq = (eq4 >> (3 - ((uint32_t)c - before_t))) & 1u;
            if (has_t && !cells_t && !eq) o->fill |= 1u << c;  // uniform, not "equal" (log.rs:452-467)
            else n.bs = 1 + rsc * 4;
        } else {
            n.bt = 1 + rtc * 4;
            n.bs = 1 + rsc * 4;
        }
    }
}
// (k = 2, items of at most 64 x 64 cells: they meet at most 5 x 5 nodes of side 16, 9 x 9 of side 8, 17 x 17 of side 4 -- 395
//  frontier entries below the top table; walking from the root adds at most 1 + 4 + 4 + 9 above them)
constexpr int WQ2_CAP = 448;
template <class V>
struct WaveQ2T {
    uint32_t it[WQ2_CAP], is[WQ2_CAP], org[WQ2_CAP];
    V mt[WQ2_CAP], ms[WQ2_CAP];
};
typedef WaveQ2T<int64_t> WaveQ2;

}  // namespace k2r
