// k2r_query_types.h -- what the query-side translation units share: the device-visible chunk handle with its side-16
// tables, and the k = 2 node-wise readers of the serialized streams (four adjacent children per lane).
#pragma once
#include <type_traits>

#include "k2r_decode.h"

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

}  // namespace k2r
