// k2r_open.hip -- C ABI, query side: opening chunks.  The parser of the serialized stream (on the host for dcdf_chunk_open, one
// thread per chunk for streams already in device memory), the structural validation, the side-16 tables the node-wise walks
// start from, and the handle's metadata.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "k2r_decode.h"
#include "k2r_query_host.h"

using namespace k2r;

namespace k2r {

// ---- host-side parser (chunk.rs:247-266, block.rs:99-109, snapshot.rs:62-81, log.rs:68-89,
//      bitmap.rs:142-164, dac.rs:48-63): records byte offsets instead of materialising vectors ----
struct Cursor {
    const uint8_t* p;
    size_t n, pos = 0;
    bool ok = true;
    K2R_HD bool need(size_t k) {
        if (!ok || pos + k > n || pos + k < pos) ok = false;
        return ok;
    }
    K2R_HD uint8_t u8() { return need(1) ? p[pos++] : 0; }
    K2R_HD uint32_t u32() {
        if (!need(4)) return 0;
        uint32_t v = load_be32(p + pos);
        pos += 4;
        return v;
    }
    K2R_HD void skip(size_t k) {
        if (need(k)) pos += k;
    }
};
K2R_HD void parse_bitmap(Cursor& c, BmDesc& d) {
    d.len = c.u32();
    d.k = c.u32();
    if (d.k == 0) c.ok = false;
    if (!c.ok) return;
    d.idx_off = (uint32_t)c.pos;
    c.skip(4ull * (d.len / 32 / d.k));
    d.words_off = (uint32_t)c.pos;
    c.skip(4ull * ((d.len + 31) / 32));
}
K2R_HD void parse_dac(Cursor& c, DacDesc& d) {
    d = DacDesc{};
    d.nlev = c.u8();
    if (d.nlev > 8) c.ok = false;
    for (uint32_t l = 0; l < d.nlev && c.ok; l++) {
        parse_bitmap(c, d.bm[l]);
        d.bytes_off[l] = (uint32_t)c.pos;
        c.skip(d.bm[l].len);
    }
}
K2R_HD void parse_inst(Cursor& c, InstDesc& d, bool is_log, uint32_t snap) {
    d = InstDesc{};
    d.is_log = is_log ? 1u : 0u;
    d.snap = snap;
    d.k = c.u8();
    d.rows = c.u32();
    d.cols = c.u32();
    d.sidelen = c.u32();
    if (d.k < 2 || d.sidelen == 0) c.ok = false;
    parse_bitmap(c, d.T);
    if (is_log) parse_bitmap(c, d.E);
    parse_dac(c, d.mx);
    parse_dac(c, d.mn);
}

// The walk's state at every node of side 16, for every instant of one chunk (dcdf_chunk::d_top): one wave per instant walks
// the top of the tree(s) breadth-first -- 1, 4, 16, ... nodes -- with the same expand4 as the query walks.
__device__ __forceinline__ void top_table_inst(const ChunkRef& C, const uint32_t inst, TopEnt* __restrict__ table, TopMM* __restrict__ table_mm,
                                               uint32_t* __restrict__ overflow, WaveQ2& q, int64_t* qmt, int64_t* qms) {
    const int lane = threadIdx.x;
    const uint32_t G = C.top_g;
    const uint8_t* const b = C.bytes;
    const gbytes gb = (gbytes)C.bytes;
    const gdesc gD = (gdesc)C.descs + inst;
    const bool has_log = gD->is_log != 0;
    const gdesc gS = has_log ? (gdesc)C.descs + gD->snap : gD;
    const InstDesc& D = C.descs[inst];
    const InstDesc& SD = has_log ? C.descs[gD->snap] : D;
    const TreeRef S = tree_ref(gS), L = tree_ref(gD);
    TopEnt* const out = table + (size_t)inst * G * G;
    TopMM* const omm = table_mm + (size_t)inst * G * G;
    // every 16-square of the node at (r, c), side sd: the walk's state there and the range of the values inside
    auto put_square = [&](uint32_t r, uint32_t c, uint32_t sd, uint32_t bt, uint32_t bs, int64_t mt, int64_t ms, int64_t vmin, int64_t vmax) {
        if (mt != (int32_t)mt || ms != (int32_t)ms || vmin != (int32_t)vmin || vmax != (int32_t)vmax) *overflow = 1;
        const TopEnt e{bt, bs, (int32_t)mt, (int32_t)ms};
        const TopMM m{(int32_t)vmin, (int32_t)vmax};
        const uint32_t n = sd >> 4;
        for (uint32_t i = 0; i < n * n; i++) {
            const uint32_t at = ((r >> 4) + i / n) * G + (c >> 4) + i % n;
            out[at] = e;
            omm[at] = m;
        }
    };
    const bool single_s = !gbm_get(gb, S.T, 0);
    const bool single_t = has_log ? !gbm_get(gb, L.T, 0) : true;
    const int64_t max_s0 = dacd_get(b, SD.mx, 0), max_t0 = has_log ? dacd_get(b, D.mx, 0) : 0;
    const int64_t min_s0 = dacd_get(b, SD.mn, 0), min_t0 = has_log ? dacd_get(b, D.mn, 0) : 0;
    const bool all_one = has_log ? (single_t && (single_s || !gbm_get(gb, L.E, 0))) : single_s;
    if (all_one) {
        if (lane == 0) put_square(0, 0, G * 16, WQ_NONE, WQ_NONE, max_t0, max_s0, max_t0 + max_s0, max_t0 + max_s0);
        return;
    }
    if (lane == 0) {
        q.it[0] = (has_log && !single_t) ? 1u : WQ_NONE;
        q.is[0] = single_s ? WQ_NONE : 1u;
        q.org[0] = 0;
        q.mt[0] = max_t0;
        q.ms[0] = max_s0;
        qmt[0] = min_t0;
        qms[0] = min_s0;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t lo = 0, hi = 1;
    for (uint32_t side = gD->sidelen; side > 16; side >>= 1) {  // (at most 64 nodes of side 32 at the last step: one pass per level)
        const uint32_t cs = side >> 1, n = lo + (uint32_t)lane;
        const bool live = n < hi;
        Kids kd;
        kd.fill = 0;
        uint32_t po = 0;
        NodeSt p{WQ_NONE, WQ_NONE, 0, 0};
        int64_t pmin_t = 0, pmin_s = 0;
        if (live) {
            p = NodeSt{q.it[n], q.is[n], q.mt[n], q.ms[n]};
            pmin_t = qmt[n];
            pmin_s = qms[n];
            po = q.org[n];
            expand4(gb, S, SD.mx, L, D.mx, p, &kd);
        }
        const uint32_t pushm = live ? (~kd.fill & 15u) : 0u, np = popc32(pushm);
        const uint32_t inc = GpuExecScan::incl(np);
        uint32_t pos = hi + inc - np;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (!live) continue;
            const uint32_t cr = (po >> 16) + (uint32_t)(c >> 1) * cs, cc = (po & 0xffffu) + (uint32_t)(c & 1) * cs;
            // the child's minima, as the reference's search carries them (log.rs:640-676; snapshot.rs:391 without a log)
            const bool has_t = p.bt != WQ_NONE, has_s = p.bs != WQ_NONE;
            const uint32_t it_ = has_t ? p.bt + (uint32_t)c : 0u, is_ = has_s ? p.bs + (uint32_t)c : 0u;
            const bool leaf_t = has_t ? (it_ >= D.T.len || !bmd_get(b, D.T, it_)) : true;
            const bool leaf_s = has_s ? (is_ >= SD.T.len || !bmd_get(b, SD.T, is_)) : true;
            const int64_t mt_ = kd.st[c].mt, ms_ = kd.st[c].ms;
            int64_t min_t_ = has_t ? (leaf_t ? pmin_t : dacd_get(b, D.mn, bmd_rank(b, D.T, it_))) : pmin_t;
            int64_t min_s_ = has_s ? (leaf_s ? pmin_s : pmin_s + dacd_get(b, SD.mn, bmd_rank(b, SD.T, is_))) : pmin_s;
            if (leaf_s) min_s_ = ms_;
            if (leaf_t) {
                min_t_ = mt_;
                if (has_t && it_ < D.T.len && !bmd_get(b, D.E, bmd_rank0(b, D.T, it_ + 1) - 1)) min_t_ = ms_ + mt_ - min_s_;
            }
            const int64_t vmax = ms_ + mt_, vmin = min_s_ + min_t_;
            if ((kd.fill >> c) & 1u) {
                put_square(cr, cc, cs, WQ_NONE, WQ_NONE, mt_, ms_, vmax, vmax);
            } else if (cs == 16) {
                put_square(cr, cc, 16, kd.st[c].bt, kd.st[c].bs, mt_, ms_, vmin, vmax);
            } else {
                q.it[pos] = kd.st[c].bt; q.is[pos] = kd.st[c].bs; q.org[pos] = (cr << 16) | cc; q.mt[pos] = mt_; q.ms[pos] = ms_;
                qmt[pos] = min_t_;
                qms[pos] = min_s_;
                pos++;
            }
        }
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        __builtin_amdgcn_wave_barrier();
        lo = hi;
        hi = cs == 16 ? hi : hi + tot;
    }
}
__global__ void __launch_bounds__(64)
k_top_table(ChunkRef C, TopEnt* __restrict__ table, TopMM* __restrict__ table_mm, uint32_t* __restrict__ overflow) {
    __shared__ WaveQ2 q;
    __shared__ int64_t qmt[WQ2_CAP], qms[WQ2_CAP];  // the frontier nodes' min_t, min_s (log.rs:360-361)
    top_table_inst(C, blockIdx.x, table, table_mm, overflow, q, qmt, qms);
}
// the same for every instant of MANY chunks in one launch (dcdf_chunk_open_batch): workgroup = one (chunk, instant);
// inst_chunk[global instant] = its chunk, first_inst[chunk] = the chunk's first global instant; each chunk's tables are where
// its ChunkRef says; overflow[chunk] != 0 afterwards = a value beyond int32 (that chunk is then walked from the root)
__global__ void __launch_bounds__(64)
k_top_table_batch(const ChunkRef* __restrict__ refs, const uint32_t* __restrict__ inst_chunk, const uint32_t* __restrict__ first_inst,
                  uint32_t* __restrict__ overflow) {
    __shared__ WaveQ2 q;
    __shared__ int64_t qmt[WQ2_CAP], qms[WQ2_CAP];
    const uint32_t ci = inst_chunk[blockIdx.x];
    const ChunkRef C = refs[ci];
    if (C.top_g == 0) return;
    top_table_inst(C, blockIdx.x - first_inst[ci], (TopEnt*)C.top, (TopMM*)C.top_mm, overflow + ci, q, qmt, qms);
}

// ---- opening chunks whose bytes are already in device memory: the parse of chunk.rs:247-266 by one thread per chunk ----
struct OpenMeta {
    uint32_t ok, encoding, fbits, n_blocks, n_inst, k, rows, cols, sidelen, narrow32;
};
// count != 0: only count the instants (descs may be null); else fill descs[first[i] ..] and the per-instant quirk flags
__global__ void __launch_bounds__(64)
k_parse_chunks(const uint8_t* __restrict__ slab, const uint64_t* __restrict__ offs, const uint64_t* __restrict__ lens, uint32_t n,
               const uint32_t* __restrict__ first, InstDesc* __restrict__ descs, uint8_t* __restrict__ quirk, OpenMeta* __restrict__ meta,
               int count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* const b = slab + offs[i];
    Cursor cur{b, (size_t)lens[i]};
    OpenMeta m{};
    m.encoding = cur.u8();
    m.fbits = cur.u8();
    m.n_blocks = cur.u32();
    bool ok = m.encoding == DCDF_I32 || m.encoding == DCDF_I64 || m.encoding == DCDF_F32 || m.encoding == DCDF_F64;
    uint32_t ni = 0;
    InstDesc* const D = count ? nullptr : descs + first[i];
    bool narrow = true;
    for (uint32_t blk = 0; blk < m.n_blocks && cur.ok && ok; blk++) {
        const uint32_t n_inst = cur.u8();  // block.rs:100
        if (n_inst == 0) ok = false;
        const uint32_t snap = ni;
        for (uint32_t j = 0; j < n_inst && cur.ok && ok; j++, ni++) {
            InstDesc d;
            parse_inst(cur, d, j > 0, snap);
            if (!cur.ok) break;
            if (ni == 0) {
                m.k = d.k; m.rows = d.rows; m.cols = d.cols; m.sidelen = d.sidelen;
            } else if (d.k != m.k || d.rows != m.rows || d.cols != m.cols || d.sidelen != m.sidelen) ok = false;
            if (d.T.k != 4 || (d.is_log && d.E.k != 4) || d.rows == 0 || d.cols == 0 || d.sidelen < (d.rows > d.cols ? d.rows : d.cols)) ok = false;
            if (!count && ok) {
                D[ni] = d;
                int64_t hi = dacd_get(b, d.mx, 0), lo = dacd_get(b, d.mn, 0);
                if (d.is_log) {  // log roots are differences against the snapshot's (log.rs:133,148)
                    hi += dacd_get(b, D[snap].mx, 0);
                    lo += dacd_get(b, D[snap].mn, 0);
                }
                const int64_t lim = (int64_t)1 << 30;
                if (hi < -lim || hi >= lim || lo < -lim || lo >= lim) narrow = false;
                quirk[first[i] + ni] = (d.is_log && !bmd_get(b, d.T, 0) && !bmd_get(b, d.E, 0) && bmd_get(b, D[snap].T, 0)) ? 1 : 0;
            }
        }
    }
    m.ok = (ok && cur.ok && ni > 0 && cur.pos == lens[i]) ? 1u : 0u;
    m.n_inst = ni;
    m.narrow32 = narrow ? 1u : 0u;
    meta[i] = m;
}
// Structural validation of the instants k_parse_chunks described: the checks dcdf_chunk_open makes on the host (every count a
// decoder relies on against the bitmaps' popcounts, the rank index of every BitMap), by one wave per instant.  bad[chunk] != 0
// afterwards: the stream is not a chunk of this format; its handle is refused before any walk chases its indices.
__device__ uint64_t wave_ones(const uint8_t* b, const BmDesc& d, bool& index_ok) {  // popcount of the bitmap (all lanes get it)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t W = (d.len + 31) / 32, nidx = d.len / 128;  // bitmap.rs:70
    uint32_t base = 0;
    for (uint32_t g0 = 0; 4 * g0 < W; g0 += 64) {  // a lane per group of four words = per entry of the rank index
        const uint32_t g = g0 + lane;
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t w = 4 * g + i;
            if (w < W) {
                uint32_t x = load_be32(b + d.words_off + 4 * w);
                const uint32_t left = d.len - 32 * w;
                if (left < 32) x &= ~(0xffffffffu >> left);  // padding bits do not count
                cnt += popc32(x);
            }
        }
        const uint32_t inc = GpuExecScan::incl(cnt);
        if (d.k == 4 && g < nidx && load_be32(b + d.idx_off + 4 * g) != base + inc) index_ok = false;  // bitmap.rs:97-104
        base += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    return base;
}
__device__ bool wave_dac_ok(const uint8_t* b, const DacDesc& d, uint64_t expect_len, bool& index_ok) {
    if (expect_len == 0) return d.nlev == 0;
    if (d.nlev == 0 || d.nlev > 8 || d.bm[0].len != expect_len) return false;
    for (uint32_t l = 0; l < d.nlev; l++) {
        if (d.bm[l].k != 4) return false;
        const uint64_t next = wave_ones(b, d.bm[l], index_ok);
        if (l + 1 < d.nlev ? d.bm[l + 1].len != next : next != 0) return false;  // dac.rs:83-90: every hop lands in the next plane
    }
    return true;
}
__global__ void __launch_bounds__(64)
k_validate_insts(const uint8_t* __restrict__ slab, const uint64_t* __restrict__ offs, const uint32_t* __restrict__ inst_chunk,
                 const InstDesc* __restrict__ descs, uint32_t* __restrict__ bad) {
    const uint32_t ci = inst_chunk[blockIdx.x];
    const uint8_t* const b = slab + offs[ci];
    const InstDesc& d = descs[blockIdx.x];
    bool index_ok = true, ok = true;
    if (d.k < 2 || d.k > 255 || d.rows == 0 || d.cols == 0 || d.T.k != 4 || (d.is_log && d.E.k != 4)) ok = false;
    if (ok) {
        const uint64_t internal = wave_ones(b, d.T, index_ok);
        const uint64_t visited = 1 + (uint64_t)d.k * d.k * internal;  // snapshot.rs:177: k^2 children per internal node
        if (d.T.len > visited) ok = false;
        if (ok && (!wave_dac_ok(b, d.mx, visited, index_ok) || !wave_dac_ok(b, d.mn, internal, index_ok))) ok = false;
        if (ok && d.is_log) {
            if (d.E.len != d.T.len - internal) ok = false;  // one eqB bit per T = 0 (log.rs:137-144)
            else (void)wave_ones(b, d.E, index_ok);
        }
    }
    if (__ballot(!ok || !index_ok) != 0 && (threadIdx.x & 63u) == 0) atomicOr(&bad[ci], 1u);
}
// encoded chunks, wherever they lie in device memory, into one slab (16-byte aligned starts)
struct SlabItem {
    const uint8_t* src;
    uint64_t len, dst_off;
};
__global__ void __launch_bounds__(256) k_slab_pack(const SlabItem* __restrict__ items, uint32_t n, uint8_t* __restrict__ dst) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const SlabItem it = items[i];
        if (((uintptr_t)it.src & 15u) == 0) {
            const uint4* s4 = (const uint4*)it.src;
            uint4* d4 = (uint4*)(dst + it.dst_off);
            const uint64_t nv = it.len / 16;
            for (uint64_t v = threadIdx.x; v < nv; v += blockDim.x) d4[v] = s4[v];
            for (uint64_t b = 16 * nv + threadIdx.x; b < it.len; b += blockDim.x) dst[it.dst_off + b] = it.src[b];
        } else {
            for (uint64_t b = threadIdx.x; b < it.len; b += blockDim.x) dst[it.dst_off + b] = it.src[b];
        }
    }
}

}  // namespace k2r

// ---- open / close / info -----------------------------------------------------------------------------
extern "C" int dcdf_chunk_open(const uint8_t* bytes, size_t len, dcdf_chunk** h) {
    if (!bytes || !h || len < 6 || len > 0xfffffff0ull) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    std::unique_ptr<dcdf_chunk> c(new (std::nothrow) dcdf_chunk());
    if (!c) return DCDF_ERR_NOMEM;
    Cursor cur{bytes, len};
    c->encoding = cur.u8();
    if (c->encoding != DCDF_I32 && c->encoding != DCDF_I64 && c->encoding != DCDF_F32 && c->encoding != DCDF_F64)
        return DCDF_ERR_FORMAT;  // mmstruct.rs:49-57
    c->fbits = cur.u8();
    c->n_blocks = cur.u32();
    for (uint32_t b = 0; b < c->n_blocks && cur.ok; b++) {
        const uint32_t n_inst = cur.u8();  // block.rs:100
        if (n_inst == 0) cur.ok = false;
        const uint32_t snap = (uint32_t)c->descs.size();
        for (uint32_t i = 0; i < n_inst && cur.ok; i++) {
            InstDesc d;
            parse_inst(cur, d, i > 0, snap);
            c->descs.push_back(d);
        }
    }
    if (!cur.ok || c->descs.empty() || cur.pos != len) return DCDF_ERR_FORMAT;
    // Structural validation (chunks arrive by CID from an untrusted store; the reference would panic on a malformed one, the
    // GPU must not chase out-of-range indices): every count the decoders rely on is checked against the bitmaps' popcounts.
    {
        bool index_ok = true;
        auto ones = [&](const BmDesc& d) -> uint64_t {  // popcount of the bitmap; checks its rank index on the way (bitmap.rs:97-104)
            uint64_t n = 0;
            for (uint32_t w = 0; w < (d.len + 31) / 32; w++) {
                uint32_t x = load_be32(bytes + d.words_off + 4 * w);
                const uint32_t left = d.len - 32 * w;
                if (left < 32) x &= ~(0xffffffffu >> left);  // padding bits do not count
                n += (uint64_t)__builtin_popcount(x);
                if (d.k == 4 && (w & 3) == 3 && (w >> 2) < d.len / 128 && load_be32(bytes + d.idx_off + 4 * (w >> 2)) != (uint32_t)n) index_ok = false;
            }
            return n;
        };
        auto dac_ok = [&](const DacDesc& d, uint64_t expect_len) -> bool {
            if (expect_len == 0) return d.nlev == 0;
            if (d.nlev == 0 || d.bm[0].len != expect_len) return false;
            for (uint32_t l = 0; l < d.nlev; l++) {
                if (d.bm[l].k != 4) return false;
                const uint64_t next = ones(d.bm[l]);
                if (l + 1 < d.nlev ? d.bm[l + 1].len != next : next != 0) return false;  // dac.rs:83-90: every hop lands in the next plane
            }
            return true;
        };
        for (const InstDesc& d : c->descs) {
            if (d.k < 2 || d.k > 255 || d.rows == 0 || d.cols == 0) return DCDF_ERR_FORMAT;
            // snapshot.rs:118-119: k^ceil(ln(max)/ln(k)) in f64 -- what the reference writes (625 for a 125-wide tile with k = 5)
            if (d.sidelen != ref_sidelen(std::max(d.rows, d.cols), d.k)) return DCDF_ERR_FORMAT;
            if (d.T.k != 4 || (d.is_log && d.E.k != 4)) return DCDF_ERR_FORMAT;  // bitmap.rs:69,130
            const uint64_t internal = ones(d.T);
            const uint64_t visited = 1 + (uint64_t)d.k * d.k * internal;          // snapshot.rs:177: four children per internal node
            if (d.T.len > visited) return DCDF_ERR_FORMAT;
            if (!dac_ok(d.mx, visited) || !dac_ok(d.mn, internal)) return DCDF_ERR_FORMAT;
            if (d.is_log && d.E.len != d.T.len - internal) return DCDF_ERR_FORMAT;  // one eqB bit per T = 0 (log.rs:137-144)
            if (d.is_log) (void)ones(d.E);
            if (!index_ok) return DCDF_ERR_FORMAT;
        }
    }
    c->instants = (uint32_t)c->descs.size();
    c->k0 = c->descs[0].k;
    c->sidelen0 = c->descs[0].sidelen;
    c->rows = c->descs[0].rows;  // chunk.rs:119-123
    c->cols = c->descs[0].cols;
    for (const InstDesc& d : c->descs)
        if (d.rows != c->rows || d.cols != c->cols || d.k != c->descs[0].k || d.sidelen != c->descs[0].sidelen ||
            d.sidelen < std::max(d.rows, d.cols))
            return DCDF_ERR_FORMAT;
    c->len = len;
    c->narrow32 = true;
    for (size_t i = 0; i < c->descs.size(); i++) {
        const InstDesc& D = c->descs[i];
        int64_t hi = dacd_get(bytes, D.mx, 0), lo = dacd_get(bytes, D.mn, 0);
        if (D.is_log) {  // log roots are differences against the snapshot's (log.rs:133,148)
            hi += dacd_get(bytes, c->descs[D.snap].mx, 0);
            lo += dacd_get(bytes, c->descs[D.snap].mn, 0);
        }
        const int64_t lim = (int64_t)1 << 30;
        if (hi < -lim || hi >= lim || lo < -lim || lo >= lim) c->narrow32 = false;
    }
    c->search_quirk.assign(c->descs.size(), 0);
    for (size_t i = 0; i < c->descs.size(); i++) {
        const InstDesc& L = c->descs[i];
        if (L.is_log && !bmd_get(bytes, L.T, 0) && !bmd_get(bytes, L.E, 0) && bmd_get(bytes, c->descs[L.snap].T, 0)) c->search_quirk[i] = 1;
    }
    K2R_HIP(c->d_bytes.alloc(len + 64));  // (slack: the wave decoder reads whole 16-byte blocks / 4-byte groups at the tail)
    K2R_HIP(hipMemcpy(c->d_bytes.p, bytes, len, hipMemcpyHostToDevice));
    K2R_HIP(upload(c->d_descs, c->descs));
    if (c->descs[0].k == 2 && c->descs[0].sidelen >= 32 && c->descs[0].sidelen <= 256 && !std::getenv("K2R_NO_TOP_TABLE")) {
        const uint32_t g = c->descs[0].sidelen / 16;
        const size_t tbytes = (size_t)c->instants * g * g * sizeof(TopEnt);
        K2R_HIP(c->d_top_mm.alloc((size_t)c->instants * g * g * sizeof(TopMM)));
        K2R_HIP(c->d_top.alloc(tbytes + 4));  // (+ the "a value does not fit int32" word)
        uint32_t* const d_ovf = (uint32_t*)(c->d_top.as<uint8_t>() + tbytes);
        K2R_HIP(hipMemset(d_ovf, 0, 4));
        ChunkRef ref{c->d_bytes.as<uint8_t>(), c->d_descs.as<InstDesc>(), c->instants, c->rows, c->cols, c->fbits, nullptr, nullptr, g, 0};
        hipLaunchKernelGGL(k_top_table, dim3(c->instants), dim3(64), 0, 0, ref, c->d_top.as<TopEnt>(), c->d_top_mm.as<TopMM>(), d_ovf);
        K2R_HIP(hipGetLastError());
        uint32_t ovf = 0;
        K2R_HIP(hipMemcpy(&ovf, d_ovf, 4, hipMemcpyDeviceToHost));
        if (!ovf) c->top_g = g;
    }
    c->p_bytes = c->d_bytes.as<uint8_t>();
    c->p_descs = c->d_descs.as<InstDesc>();
    c->p_top = c->d_top.p;
    c->p_top_mm = c->d_top_mm.p;
    *h = c.release();
    return DCDF_OK;
}
extern "C" void dcdf_chunk_close(dcdf_chunk* h) { delete h; }

namespace {
struct BatchSlab {  // what the chunks of one dcdf_chunk_open_batch share
    DevBuf bytes, descs, top, top_mm, refs;
};
}  // namespace

// Many chunks at once.  mem = DCDF_MEM_HOST: dcdf_chunk_open one by one (full structural validation).  mem = DCDF_MEM_DEVICE:
// the bytes are where an encoder session left them (dcdf_encoder_result's device pointers) -- they are packed into one slab,
// parsed ON the device (k_parse_chunks, one thread per chunk: bounds-checked walk of the same layout, no host copy of the
// bytes), and the side-16 tables of all their instants are built by ONE launch (k_top_table_batch, a wave per instant).
// Device input gets the same structural validation as dcdf_chunk_open's (k_validate_insts: popcounts against the Dac and eqB
// lengths, rank indexes), a wave per instant.  status (may be NULL) receives one code per chunk; out[i] is NULL where it is not 0.
extern "C" int dcdf_chunk_open_batch(const uint8_t* const* bytes, const uint64_t* lens, size_t n, int mem, dcdf_chunk** out,
                                     int32_t* status) {
    if (!bytes || !lens || !out || n == 0 || n > 0x7fffffffu || (mem != DCDF_MEM_HOST && mem != DCDF_MEM_DEVICE)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    for (size_t i = 0; i < n; i++) out[i] = nullptr;
    if (mem == DCDF_MEM_HOST) {
        int first_err = DCDF_OK;
        for (size_t i = 0; i < n; i++) {
            const int rc = dcdf_chunk_open(bytes[i], (size_t)lens[i], &out[i]);
            if (status) status[i] = rc;
            if (rc != DCDF_OK && first_err == DCDF_OK) first_err = rc;
        }
        return status ? DCDF_OK : first_err;
    }
    struct OpenTimer {  // K2R_OPEN_TIMING=1: wall time of the steps on stderr (diagnostics; the laps synchronise the device)
        const bool on = std::getenv("K2R_OPEN_TIMING") != nullptr;
        std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
        void lap(const char* what) {
            if (!on) return;
            (void)hipDeviceSynchronize();
            const auto u = std::chrono::steady_clock::now();
            std::fprintf(stderr, "k2r-open %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(u - t).count());
            t = u;
        }
    } tm;
    auto slab = std::make_shared<BatchSlab>();
    std::vector<SlabItem> items(n);
    std::vector<uint64_t> offs(n);
    uint64_t tot = 0;
    for (size_t i = 0; i < n; i++) {
        if (!bytes[i] || lens[i] < 6 || lens[i] > 0xfffffff0ull) return DCDF_ERR_BAD_ARG;
        offs[i] = tot;
        items[i] = SlabItem{bytes[i], lens[i], tot};
        tot += (lens[i] + 64 + 15) & ~15ull;  // (slack: the wave decoder reads whole 16-byte blocks at a stream's tail)
    }
    DevBuf d_items, d_offs, d_lens, d_first, d_meta, d_quirk, d_ic, d_ovf;
    K2R_HIP(slab->bytes.alloc_pooled(tot));  // (gigabytes: hipMalloc takes 4 .. 60 ms for them, depending on what the driver has to clear)
    K2R_HIP(upload(d_items, items));
    hipLaunchKernelGGL(k_slab_pack, dim3((uint32_t)std::min<size_t>(n, 8192)), dim3(256), 0, 0, d_items.as<SlabItem>(), (uint32_t)n,
                       slab->bytes.as<uint8_t>());
    K2R_HIP(hipGetLastError());
    tm.lap("slab alloc + pack");
    K2R_HIP(upload(d_offs, offs));
    K2R_HIP(upload(d_lens, lens, n * 8));
    K2R_HIP(d_meta.alloc(n * sizeof(OpenMeta)));
    const uint32_t pgrid = (uint32_t)((n + 63) / 64);
    // pass 1: instants per chunk
    hipLaunchKernelGGL(k_parse_chunks, dim3(pgrid), dim3(64), 0, 0, slab->bytes.as<uint8_t>(), d_offs.as<uint64_t>(), d_lens.as<uint64_t>(),
                       (uint32_t)n, (const uint32_t*)nullptr, (InstDesc*)nullptr, (uint8_t*)nullptr, d_meta.as<OpenMeta>(), 1);
    K2R_HIP(hipGetLastError());
    std::vector<OpenMeta> meta(n);
    K2R_HIP(hipMemcpy(meta.data(), d_meta.p, n * sizeof(OpenMeta), hipMemcpyDeviceToHost));
    tm.lap("parse pass 1");
    std::vector<uint32_t> first(n + 1, 0);
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + (meta[i].ok ? meta[i].n_inst : 0u);
    const uint32_t total_inst = first[n];
    if (total_inst == 0) {
        if (status) for (size_t i = 0; i < n; i++) status[i] = DCDF_ERR_FORMAT;
        return status ? DCDF_OK : DCDF_ERR_FORMAT;
    }
    // pass 2: the descriptors (chunks that failed pass 1 get a zero-length stream: parsed as malformed again, nothing stored)
    std::vector<uint64_t> lens2(lens, lens + n);
    for (size_t i = 0; i < n; i++)
        if (!meta[i].ok) lens2[i] = 0;
    K2R_HIP(hipMemcpy(d_lens.p, lens2.data(), n * 8, hipMemcpyHostToDevice));
    K2R_HIP(upload(d_first, first));
    K2R_HIP(slab->descs.alloc((size_t)total_inst * sizeof(InstDesc)));
    K2R_HIP(d_quirk.alloc(total_inst));
    hipLaunchKernelGGL(k_parse_chunks, dim3(pgrid), dim3(64), 0, 0, slab->bytes.as<uint8_t>(), d_offs.as<uint64_t>(), d_lens.as<uint64_t>(),
                       (uint32_t)n, d_first.as<uint32_t>(), slab->descs.as<InstDesc>(), d_quirk.as<uint8_t>(), d_meta.as<OpenMeta>(), 0);
    K2R_HIP(hipGetLastError());
    std::vector<OpenMeta> meta2(n);
    K2R_HIP(hipMemcpy(meta2.data(), d_meta.p, n * sizeof(OpenMeta), hipMemcpyDeviceToHost));
    std::vector<uint8_t> quirk(total_inst);
    K2R_HIP(hipMemcpy(quirk.data(), d_quirk.p, total_inst, hipMemcpyDeviceToHost));
    tm.lap("parse pass 2 + descs D2H");
    // structural validation of every instant (the host entry point's checks, a wave per instant), before anything walks them
    std::vector<uint32_t> inst_chunk(total_inst);
    for (size_t i = 0; i < n; i++)
        for (uint32_t j = first[i]; j < first[i + 1]; j++) inst_chunk[j] = (uint32_t)i;
    K2R_HIP(upload(d_ic, inst_chunk));
    {
        DevBuf d_bad;
        K2R_HIP(d_bad.alloc(n * 4));
        K2R_HIP(hipMemset(d_bad.p, 0, n * 4));
        hipLaunchKernelGGL(k_validate_insts, dim3(total_inst), dim3(64), 0, 0, slab->bytes.as<uint8_t>(), d_offs.as<uint64_t>(), d_ic.as<uint32_t>(),
                           slab->descs.as<InstDesc>(), d_bad.as<uint32_t>());
        K2R_HIP(hipGetLastError());
        std::vector<uint32_t> bad(n);
        K2R_HIP(hipMemcpy(bad.data(), d_bad.p, n * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++)
            if (bad[i]) meta2[i].ok = 0;
    }
    tm.lap("validation");
    // side-16 tables for the k = 2 chunks of sidelen 32..256: one slab, one launch
    const bool want_top = !std::getenv("K2R_NO_TOP_TABLE");
    std::vector<uint64_t> top_off(n, 0);
    std::vector<uint32_t> top_g(n, 0);
    uint64_t squares = 0;
    for (size_t i = 0; i < n; i++) {
        if (!meta[i].ok || !meta2[i].ok) continue;
        // the depth the reference computes (k2r_runtime.h ref_sidelen): a stream that disagrees is not a chunk of this format
        if (meta[i].sidelen != ref_sidelen(std::max(meta[i].rows, meta[i].cols), meta[i].k)) {
            meta2[i].ok = 0;
            continue;
        }
        if (want_top && meta[i].k == 2 && meta[i].sidelen >= 32 && meta[i].sidelen <= 256) {
            top_g[i] = meta[i].sidelen / 16;
            top_off[i] = squares;
            squares += (uint64_t)meta[i].n_inst * top_g[i] * top_g[i];
        }
    }
    std::vector<ChunkRef> refs(n);
    if (squares) {
        K2R_HIP(slab->top.alloc(squares * sizeof(TopEnt)));
        K2R_HIP(slab->top_mm.alloc(squares * sizeof(TopMM)));
    }
    for (size_t i = 0; i < n; i++) {
        const bool ok = meta[i].ok && meta2[i].ok;
        refs[i] = ChunkRef{slab->bytes.as<uint8_t>() + offs[i], slab->descs.as<InstDesc>() + first[i], ok ? meta[i].n_inst : 0u, meta[i].rows,
                           meta[i].cols, meta[i].fbits, top_g[i] ? slab->top.as<TopEnt>() + top_off[i] : nullptr,
                           top_g[i] ? slab->top_mm.as<TopMM>() + top_off[i] : nullptr, ok ? top_g[i] : 0u, 0};
    }
    K2R_HIP(upload(slab->refs, refs));
    std::vector<uint32_t> ovf(n, 0);
    if (squares) {
        K2R_HIP(d_ovf.alloc(n * 4));
        K2R_HIP(hipMemset(d_ovf.p, 0, n * 4));
        hipLaunchKernelGGL(k_top_table_batch, dim3(total_inst), dim3(64), 0, 0, slab->refs.as<ChunkRef>(), d_ic.as<uint32_t>(), d_first.as<uint32_t>(),
                           d_ovf.as<uint32_t>());
        K2R_HIP(hipGetLastError());
        K2R_HIP(hipMemcpy(ovf.data(), d_ovf.p, n * 4, hipMemcpyDeviceToHost));
    }
    tm.lap("top tables");
    K2R_HIP(hipDeviceSynchronize());
    int first_err = DCDF_OK;
    for (size_t i = 0; i < n; i++) {
        const bool ok = meta[i].ok && meta2[i].ok;
        if (status) status[i] = ok ? DCDF_OK : DCDF_ERR_FORMAT;
        if (!ok) {
            if (first_err == DCDF_OK) first_err = DCDF_ERR_FORMAT;
            continue;
        }
        std::unique_ptr<dcdf_chunk> c(new (std::nothrow) dcdf_chunk());
        if (!c) {
            for (size_t j = 0; j < i; j++) {
                delete out[j];
                out[j] = nullptr;
            }
            return DCDF_ERR_NOMEM;
        }
        c->instants = meta[i].n_inst;
        c->k0 = meta[i].k;
        c->sidelen0 = meta[i].sidelen;
        c->rows = meta[i].rows;
        c->cols = meta[i].cols;
        c->n_blocks = meta[i].n_blocks;
        c->encoding = (int32_t)meta[i].encoding;
        c->fbits = meta[i].fbits;
        c->len = (size_t)lens[i];
        c->narrow32 = meta2[i].narrow32 != 0;
        c->search_quirk.assign(quirk.begin() + first[i], quirk.begin() + first[i + 1]);
        c->top_g = (top_g[i] && !ovf[i]) ? top_g[i] : 0;
        c->p_bytes = refs[i].bytes;
        c->p_descs = refs[i].descs;
        c->p_top = refs[i].top;
        c->p_top_mm = refs[i].top_mm;
        c->store = slab;
        out[i] = c.release();
    }
    tm.lap("handles");
    return status ? DCDF_OK : first_err;
}
extern "C" int dcdf_chunk_info(const dcdf_chunk* h, uint32_t shape[3], int32_t* encoding, uint32_t* fractional_bits,
                               uint32_t* n_blocks) {
    if (!h) return DCDF_ERR_BAD_ARG;
    if (shape) {
        shape[0] = h->instants;
        shape[1] = h->rows;
        shape[2] = h->cols;
    }
    if (encoding) *encoding = h->encoding;
    if (fractional_bits) *fractional_bits = h->fbits;
    if (n_blocks) *n_blocks = h->n_blocks;
    return DCDF_OK;
}

// Byte range of every instant's Snapshot / Log inside the chunk (off[i] .. off[i + 1]; off has instants + 1 entries) and
// the instant of the snapshot its block starts with: what a decode of instant i can touch at most (decode path:
// "encoded bytes of the touched chunks' touched structures").  Host metadata only.
extern "C" int dcdf_chunk_instant_layout(const dcdf_chunk* h, uint64_t* off, uint32_t* snapshot_of) {
    if (!h || !off) return DCDF_ERR_BAD_ARG;
    const std::vector<InstDesc>& descs = host_descs(h);
    if (descs.size() != h->instants) return DCDF_ERR_INTERNAL;
    for (uint32_t i = 0; i < h->instants; i++) {
        off[i] = (uint64_t)descs[i].T.idx_off - 8 - 13;  // BitMap header (len, k) and the 13-byte instant header before it
        if (snapshot_of) snapshot_of[i] = descs[i].snap;
    }
    off[h->instants] = h->len;
    return DCDF_OK;
}
