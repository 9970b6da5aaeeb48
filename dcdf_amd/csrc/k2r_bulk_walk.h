// k2r_bulk_walk.h -- the block walk all four bulk kernels of k2r_bulk.hip share (device only), written down once: the Snapshot of
// a block is decoded ONCE per region into an LDS max-pyramid, then every instant of the block is a walk of its Log's own tree
// (T, eqB, Lmax) whose leaves are filled from that pyramid.  The kernels differ only in what they do with a task's cells.
//
// Why that is the window walk's result (Log::_fill_window, log.rs:349-508): a Log node stores d = max_t - max_s itself (assigned,
// not accumulated: log.rs:397-400), so the value the lock-step descent yields over a square is always d(log leaf) + S, S being the
// Snapshot's running max_s where the descent stands:
//   * Log leaf, eqB bit 0 (uniform, log.rs:452-467): every cell of the node's square is d + max_s(same node);
//   * Log leaf with eqB bit 1, or the Log side already None: the descent goes on in the Snapshot alone with max_t fixed: every cell
//     is d + s(cell);
//   * Snapshot leaf above, Log goes on (log.rs:433-450): max_s stays the Snapshot leaf's value: every cell is d(cell-level log
//     leaf) + that value.
// So with P[l][node] = the Snapshot's own max_s of every node of side 2^l inside the region -- BELOW a Snapshot leaf the leaf's
// value repeated, filled top-down from the tree (padded squares stay exact) -- the three cases read "d + P[l][node]" (uniform leaf
// at level l) and "d + P[0][cell]" (the other two).  The root shortcuts of Log::fill_window (log.rs:315-327) are the same rule at
// the root; they and everything above side 16 come ready-made from the chunk's side-16 table (TopEnt, k_top_table).  Lmin is
// never read.
#pragma once
#include "k2r_bulk.h"

namespace k2r {

// Level l = nodes of side 2^l; the region holds (64 >> l)^2 of them, row-major.  Values of levels 0..4, walk state of levels 1..4.
constexpr uint32_t BP_OFF[5] = {0u, 4096u, 5120u, 5376u, 5440u};
constexpr uint32_t BP_SIZE = 5456u;  // 21 824 bytes of int32
constexpr uint32_t BN_OFF[5] = {0u, 336u, 80u, 16u, 0u};  // (level 0 has no state: cells)
constexpr uint32_t BN_SIZE = 1360u;
// state word of a node during a Log's walk: the index of its first child in the Log tree (open), or resolved: every cell below
// is d + P[l][its ancestor at level l] (BS_RES | l), or d itself (BS_CONST: a square the side-16 table already holds as one value)
constexpr uint32_t BS_RES = 0x80000000u, BS_CONST = BS_RES | 7u;

__device__ __forceinline__ TopEnt top_load(const TopEnt* p) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 x = *(__attribute__((address_space(1))) const u32x4*)p;
    return TopEnt{x.x, x.y, (int32_t)x.z, (int32_t)x.w};
}

// One level of the Snapshot's pyramid: a lane per node of level PL with its four adjacent children (dac4 / rank_nib); a node
// without children in the tree hands its value down.
template <int PL>
__device__ __forceinline__ void bulk_snap_level(gbytes gb, const TreeRef& S, const DacDesc& Sfull, int32_t* pyr, uint32_t* nst, uint32_t tid) {
    constexpr uint32_t WP = BULK_REGION >> PL, NP = WP * WP;
    for (uint32_t n = tid; n < NP; n += 256u) {
        const uint32_t idx = nst[BN_OFF[PL] + n];
        const int32_t pv = pyr[BP_OFF[PL] + n];
        int32_t cv[4] = {pv, pv, pv, pv};
        uint32_t ci[4] = {WQ_NONE, WQ_NONE, WQ_NONE, WQ_NONE};
        if (idx != WQ_NONE) {
            int32_t ds[4];
            dac4<int32_t>(gb, S, Sfull, idx, ds);
            uint32_t ts = 0, rs = 0;
            if (PL > 1 && idx < S.T.len) rs = rank_nib(gb, S.T, idx, &ts);  // (children beyond T are cells: snapshot.rs:281-299)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                cv[c] = pv - ds[c];
                if ((ts >> (3 - c)) & 1u) ci[c] = 1u + (rs + popc32(ts >> (4 - c))) * 4u;
            }
        }
        const uint32_t pr = n / WP, pc = n % WP;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t at = (2u * pr + (uint32_t)(c >> 1)) * (2u * WP) + 2u * pc + (uint32_t)(c & 1);
            pyr[BP_OFF[PL - 1] + at] = cv[c];
            if (PL > 1) nst[BN_OFF[PL - 1] + at] = ci[c];
        }
    }
}
// One level of a Log's walk (log.rs:392-505 without the Snapshot side): a lane per node of level PL; an open node reads its four
// children's Lmax, T and eqB bits, a resolved one hands its state down.
template <int PL>
__device__ __forceinline__ void bulk_log_level(gbytes gb, const TreeRef& L, const DacDesc& Lfull, uint32_t* nst, int32_t* nd, uint32_t tid) {
    constexpr uint32_t WP = BULK_REGION >> PL, NP = WP * WP;
    for (uint32_t n = tid; n < NP; n += 256u) {
        const uint32_t st = nst[BN_OFF[PL] + n];
        const int32_t d = nd[BN_OFF[PL] + n];
        uint32_t cs[4] = {st, st, st, st};
        int32_t cd[4] = {d, d, d, d};
        if (!(st & BS_RES)) {
            int32_t dt[4];
            dac4<int32_t>(gb, L, Lfull, st, dt);
            const bool cells = st >= L.T.len;  // (malformed: children beyond T are cells, taken as "equal" like expand4)
            uint32_t tt = 0, rt = 0, eq4 = 0xfu;
            if (!cells) {
                rt = rank_nib(gb, L.T, st, &tt);
                // eqB has one bit per T = 0 node: child c's is the (zeros among the children before c)-th from eqB[st - rt] on
                eq4 = gbm_get4(gb, L.E, st - rt);
            }
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t before = popc32(tt >> (4 - c));
                cd[c] = dt[c];
                if ((tt >> (3 - c)) & 1u) cs[c] = 1u + (rt + before) * 4u;
                else cs[c] = ((eq4 >> (3u - ((uint32_t)c - before))) & 1u) ? BS_RES : (BS_RES | (uint32_t)(PL - 1));
            }
        }
        const uint32_t pr = n / WP, pc = n % WP;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t at = (2u * pr + (uint32_t)(c >> 1)) * (2u * WP) + 2u * pc + (uint32_t)(c & 1);
            nst[BN_OFF[PL - 1] + at] = cs[c];
            nd[BN_OFF[PL - 1] + at] = cd[c];
        }
    }
}
// d + P[l][ancestor of region cell (r, c) at level l] for a resolved state word
__device__ __forceinline__ int32_t bulk_resolved(const int32_t* pyr, uint32_t st, int32_t d, uint32_t r, uint32_t c) {
    if (st == BS_CONST) return d;
    const uint32_t l = st & 7u;
    const uint32_t off = l == 0 ? BP_OFF[0] : l == 1 ? BP_OFF[1] : l == 2 ? BP_OFF[2] : l == 3 ? BP_OFF[3] : BP_OFF[4];
    return d + pyr[off + ((r >> l) << (6u - l)) + (c >> l)];
}

// What bulk_cells8 needs of the instant bulk_instant prepared: L and Lfull are only looked at when is_log.
struct BulkInstant {
    bool is_log;
    TreeRef L;
    const DacDesc* Lfull;  // (generic view: only for the rare values of three or more bytes)
};
// Instant t of unit U (any of BulkUnit, ReduceUnit, SpaceUnit, HistUnit: only rr and rc are read) down to the nodes of side 2,
// from the barrier behind the previous instant's readers to the one that publishes level 1.  On a new block (cur_snap, which the
// caller starts at 0xffffffff per unit) the Snapshot's side-16 entries and its pyramid, once; for a Log its side-16 entries and
// the levels 4..2 of its walk.  Every thread of the workgroup calls it.
template <class Unit>
__device__ __forceinline__ BulkInstant bulk_instant(const ChunkRef& C, const Unit& U, uint32_t t, uint32_t& cur_snap, int32_t* pyr, uint32_t* nst,
                                                    int32_t* nd, uint32_t tid) {
    const gbytes gb = (gbytes)C.bytes;
    const uint32_t G = C.top_g, r16 = (uint32_t)U.rr >> 4, c16 = (uint32_t)U.rc >> 4;
    const uint32_t qi = (tid >> 2) & 3u, qj = tid & 3u;  // (tid < 16: its side-16 square of the region)
    const bool sq_in = r16 + qi < G && c16 + qj < G;
    const gdesc gD = (gdesc)C.descs + t;
    const bool is_log = gD->is_log != 0;
    const uint32_t snap = is_log ? gD->snap : t;
    __syncthreads();  // (the previous instant's readers are done)
    if (snap != cur_snap) {  // a new block: its Snapshot's pyramid, once
        cur_snap = snap;
        const TreeRef S = tree_ref((gdesc)C.descs + snap);
        const DacDesc& Sfull = C.descs[snap].mx;
        if (tid < 16u) {
            int32_t v = 0;
            uint32_t idx = WQ_NONE;
            if (sq_in) {
                const TopEnt e = top_load(C.top + ((size_t)snap * G + r16 + qi) * G + c16 + qj);
                v = e.mt + e.ms;
                idx = e.bs;
            }
            pyr[BP_OFF[4] + tid] = v;
            nst[BN_OFF[4] + tid] = idx;
        }
        __syncthreads();
        bulk_snap_level<4>(gb, S, Sfull, pyr, nst, tid);
        __syncthreads();
        bulk_snap_level<3>(gb, S, Sfull, pyr, nst, tid);
        __syncthreads();
        bulk_snap_level<2>(gb, S, Sfull, pyr, nst, tid);
        __syncthreads();
        bulk_snap_level<1>(gb, S, Sfull, pyr, nst, tid);
        __syncthreads();
    }
    const BulkInstant I{is_log, tree_ref(gD), &C.descs[t].mx};
    if (is_log) {
        if (tid < 16u) {
            uint32_t st = BS_CONST;
            int32_t d = 0;
            if (sq_in) {
                const TopEnt e = top_load(C.top + ((size_t)t * G + r16 + qi) * G + c16 + qj);
                if (e.bt != WQ_NONE) {
                    st = e.bt;
                } else if (e.bs != WQ_NONE) {  // the Log ended above ("equal", or its root): mt + s(cell)
                    st = BS_RES;
                    d = e.mt;
                } else {
                    d = e.mt + e.ms;
                }
            }
            nst[BN_OFF[4] + tid] = st;
            nd[BN_OFF[4] + tid] = d;
        }
        __syncthreads();
        bulk_log_level<4>(gb, I.L, *I.Lfull, nst, nd, tid);
        __syncthreads();
        bulk_log_level<3>(gb, I.L, *I.Lfull, nst, nd, tid);
        __syncthreads();
        bulk_log_level<2>(gb, I.L, *I.Lfull, nst, nd, tid);
        __syncthreads();
    }
    return I;
}

// Task (rp, cg) of the instant, rp < 32, cg < 16: the two nodes of side 2 at node row rp, node columns 2 cg and 2 cg + 1, as
// their 2 x 4 cells v[i][e] = region cell (2 rp + i, 4 cg + e).  An open node reads its four cells' d, a resolved one (every node
// of a Snapshot instant) reads the pyramid alone.
__device__ __forceinline__ void bulk_cells8(gbytes gb, const BulkInstant& I, const int32_t* pyr, const uint32_t* nst, const int32_t* nd,
                                            uint32_t rp, uint32_t cg, int32_t (&v)[2][4]) {
#pragma unroll
    for (uint32_t j = 0; j < 2u; j++) {
        const uint32_t n = rp * 32u + 2u * cg + j;
        const uint32_t st = I.is_log ? nst[BN_OFF[1] + n] : BS_RES;
        const int32_t d = I.is_log ? nd[BN_OFF[1] + n] : 0;
        if (!(st & BS_RES)) {
            int32_t dt[4];
            dac4<int32_t>(gb, I.L, *I.Lfull, st, dt);
#pragma unroll
            for (uint32_t c = 0; c < 4u; c++)
                v[c >> 1][2u * j + (c & 1u)] = dt[c] + pyr[(2u * rp + (c >> 1)) * 64u + 4u * cg + 2u * j + (c & 1u)];
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 4u; c++)
                v[c >> 1][2u * j + (c & 1u)] = bulk_resolved(pyr, st, d, 2u * rp + (c >> 1), 4u * cg + 2u * j + (c & 1u));
        }
    }
}

// Which of the thread's 16 cells count for unit U (SpaceUnit or HistUnit): inside the unit's rectangle and, MASKED, their mask
// byte non-zero.  Bit (2 k + i) * 4 + e = cell v[i][e] of the thread's task k: (rp, cg) = (g >> 4, g & 15) of g = tid + 256 k.
template <bool MASKED, class Unit>
__device__ __forceinline__ uint32_t bulk_select16(const Unit& U, const uint8_t* mask, uint32_t tid) {
    uint32_t sel = 0;
#pragma unroll
    for (uint32_t b = 0; b < 16u; b++) {
        const uint32_t g = tid + 256u * (b >> 3), r = (uint32_t)U.rr + 2u * (g >> 4) + ((b >> 2) & 1u), c = (uint32_t)U.rc + 4u * (g & 15u) + (b & 3u);
        bool in = r >= U.top && r < U.bottom && c >= U.left && c < U.right;
        if constexpr (MASKED) {
            if (in) in = ((const __attribute__((address_space(1))) uint8_t*)mask)[U.m_off + (uint64_t)(r - U.top) * U.m_sr + (c - U.left)] != 0;
        }
        sel |= in ? 1u << b : 0u;
    }
    return sel;
}

// one workgroup per unit, the rest grid-strided
inline dim3 bulk_grid(uint32_t n_units) { return dim3(n_units < (1u << 20) ? n_units : (1u << 20)); }

}  // namespace k2r
