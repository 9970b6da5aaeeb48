// k2r_capi_encode.hip -- C ABI, the encode session (include/dcdf_k2r.h): create, run, and what reads a finished run on the
// device.  What runs where is planned in k2r_session_plan.h (plain C++, tested on the CPU); this unit allocates, turns the plan's
// offsets into pointers, launches, and applies the plan's decisions after a run.  Its two kernels splice speculative parts
// (k_stitch) and pack the slots for a gather (k_pack).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "k2r_launch.h"
#include "k2r_session.h"
#include "k2r_session_prof.h"

using namespace k2r;

namespace k2r {

// Splices the parts of a split tile: items[first[j]] = the tile (first part, in its own slot), the rest = its continuations
// in order.  Valid when the first part holds exactly one block and no middle part opened one (what every continuation
// assumed): the bytes are appended, block 0's count byte (chunk offset 6, block.rs:89) and n_blocks (chunk.rs:238) are
// patched, the counters added.  Otherwise ST_RESPLIT (the host re-encodes the tile whole); an error of any part is the
// tile's error.
constexpr int kMaxParts = 8;
// COPY = false (inside dcdf_encoder_run, timed): the checks, the totals and the two header patches -- the continuations' bytes
// stay in their own slots.  COPY = true (materialize(), the first time somebody asks for the bytes: gather, download, fetch, the
// device pointer, hashing): the bytes are appended.  The copy is 250 MB per launch for the N = 8 share of configs[3], 7 % of
// that launch, and a gather copies every byte again anyway.  TileResult::_pad2 of the first part keeps its own length between
// the two.
template <bool COPY>
__global__ void __launch_bounds__(1024) k_stitch(const uint32_t* __restrict__ first, const uint32_t* __restrict__ items,
                                                  const TileArgs* __restrict__ args, TileResult* __restrict__ res) {
    __shared__ int32_t s_st;
    __shared__ uint64_t s_at[kMaxParts + 1];
    const uint32_t i0 = first[blockIdx.x], np = first[blockIdx.x + 1] - i0;
    const uint32_t a = items[i0];
    if (threadIdx.x == 0) {
        int32_t st = ST_OK;
        uint64_t total = COPY ? (uint64_t)res[a]._pad2 : res[a].len;
        if (res[a].status != ST_OK) st = res[a].status;
        else if (!COPY && res[a].snapshots != 1) st = ST_RESPLIT;
        for (uint32_t p = 1; p < np && st == ST_OK; p++) {
            const uint32_t b = items[i0 + p];
            if (res[b].status != ST_OK) st = res[b].status;
            else if (!COPY && p + 1 < np && res[b].snapshots != 0) st = ST_RESPLIT;
            s_at[p] = total;
            total += res[b].len;
        }
        if (st == ST_OK && total > args[a].out_cap) st = ST_OUT_CAPACITY;
        s_at[np] = total;
        s_st = st;
    }
    __syncthreads();
    const int32_t st = s_st;
    if (COPY && st == ST_OK) {
        // 16 bytes per thread and step (a source slot is 256-byte aligned; the destination is wherever the previous part ended:
        // global memory takes unaligned vector stores), then the tail
        typedef uint32_t u4 __attribute__((ext_vector_type(4), aligned(1)));
        typedef uint32_t u4a __attribute__((ext_vector_type(4)));
        for (uint32_t p = 1; p < np; p++) {
            const uint32_t b = items[i0 + p];
            uint8_t* dst = args[a].out + s_at[p];
            const uint8_t* src = args[b].out;
            const uint64_t lb = s_at[p + 1] - s_at[p], nv = lb / 16;
            for (uint64_t i = threadIdx.x; i < nv; i += blockDim.x) *(u4*)(dst + 16 * i) = *(const u4a*)(src + 16 * i);
            for (uint64_t i = 16 * nv + threadIdx.x; i < lb; i += blockDim.x) dst[i] = src[i];
        }
    }
    if (!COPY && threadIdx.x == 0) {
        if (st == ST_OK) {
            const uint32_t last = items[i0 + np - 1];
            args[a].out[6] = (uint8_t)res[last].carry_count;
            store_be32(args[a].out + 2, 1u + res[last].snapshots);
            res[a]._pad2 = (uint32_t)res[a].len;  // (a slot holds far less than 4 GB)
            res[a].len = s_at[np];
            for (uint32_t p = 1; p < np; p++) {
                const uint32_t b = items[i0 + p];
                res[a].snapshots += res[b].snapshots;
                res[a].logs += res[b].logs;
                res[a].stash_logs += res[b].stash_logs;
            }
        } else {
            res[a].status = st;
            res[a].len = 0;
        }
    }
}

}  // namespace k2r

// the session's environment: read once per session (tests change it between sessions), never by the planner
static SessionKnobs read_knobs() {
    SessionKnobs kn;
    if (const char* s = std::getenv("K2R_SPLIT"))
        kn.split = std::strcmp(s, "0") == 0     ? SessionKnobs::kSplitOff
                   : std::strcmp(s, "all") == 0  ? SessionKnobs::kSplitAll
                   : std::strcmp(s, "tail") == 0 ? SessionKnobs::kSplitTail
                                                 : SessionKnobs::kSplitDefault;
    if (const char* s = std::getenv("K2R_PARTS")) kn.max_parts = (uint32_t)std::max(2, std::min(8, std::atoi(s)));
    if (const char* s = std::getenv("K2R_MAX_WGS")) kn.max_wgs = (uint32_t)std::max(1, std::atoi(s));
    if (const char* s = std::getenv("K2R_STASH_WORDS")) kn.stash_words = (uint32_t)std::atoi(s);
    return kn;
}

// what the kernels read of item `it`: the tile's descriptor, and the plan's offsets as pointers into the session's buffers
static TileArgs tile_args(const dcdf_encoder* e, const PlanItem& it, uint32_t stash_words) {
    const dcdf_tile_desc& t = e->desc[it.tile];
    TileArgs a{};
    a.stash_words = stash_words;
    a.base = t.base;
    a.st = t.stride_t; a.sr = t.stride_r; a.sc = t.stride_c;
    a.instants = t.instants; a.rows = t.rows; a.cols = t.cols;
    a.dtype = t.dtype;
    a.fbits = (t.dtype == DCDF_F32 || t.dtype == DCDF_F64) ? t.fractional_bits : 0;  // mmbuffer.rs:397-403
    a.round = t.round;
    a.out = (it.in_parts_slab ? e->d_out_b : e->d_out).as<uint8_t>() + it.out_off;
    a.out_cap = it.out_cap;
    a.minmax = e->d_minmax.as<int64_t>() + e->plan.minmax_off[it.tile];
    a.inst_begin = it.inst_begin;
    a.inst_end = it.inst_end;
    if (it.flag >= 0) {
        a.shared_flag = e->d_flags.as<uint32_t>() + 4 * it.flag;
        a.shared_cmp = (uint32_t*)(e->d_shared.as<uint8_t>() + it.shared_off);
    }
    return a;
}

static int download_results(dcdf_encoder* e) {
    K2R_HIP(hipMemcpy(e->results.data(), e->d_results.p, e->desc.size() * sizeof(TileResult), hipMemcpyDeviceToHost));
    return DCDF_OK;
}
static int upload_tile(dcdf_encoder* e, uint32_t ti) {
    K2R_HIP(hipMemcpy(e->d_args.as<TileArgs>() + ti, &e->args[ti], sizeof(TileArgs), hipMemcpyHostToDevice));
    return DCDF_OK;
}
// an output slot of `cap` bytes for tile ti alone (host mirror only: upload_tile)
static int own_slot(dcdf_encoder* e, uint32_t ti, uint64_t cap) {
    std::unique_ptr<DevBuf> b(new DevBuf());
    K2R_HIP(b->alloc(cap));
    e->args[ti].out = b->as<uint8_t>();
    e->args[ti].out_cap = cap;
    e->retry_slots.push_back(std::move(b));
    return DCDF_OK;
}
// every class's full launch order
static int upload_orders(dcdf_encoder* e) {
    const SessionPlan& p = e->plan;
    for (size_t ci = 0; ci < p.classes.size(); ci++)
        K2R_HIP(hipMemcpy(e->d_order.as<uint32_t>() + p.order_off[ci], p.class_items[ci].data(), p.class_items[ci].size() * 4,
                          hipMemcpyHostToDevice));
    return DCDF_OK;
}
// the split tiles and their parts as k_stitch<false> reads them (the tables only ever shrink: allocated the first time)
static int upload_part_tables(dcdf_encoder* e) {
    const PartTables t = part_tables(e->plan);
    if (!e->d_part_first.p) {
        K2R_HIP(e->d_part_first.alloc(t.first.size() * 4));
        K2R_HIP(e->d_part_items.alloc(t.items.size() * 4));
    }
    K2R_HIP(hipMemcpy(e->d_part_first.p, t.first.data(), t.first.size() * 4, hipMemcpyHostToDevice));
    K2R_HIP(hipMemcpy(e->d_part_items.p, t.items.data(), t.items.size() * 4, hipMemcpyHostToDevice));
    return DCDF_OK;
}
// launches() on the session's stream between its two events, waited for; *ms (if asked for) = the time between the events
template <class F>
static int timed(dcdf_encoder* e, float* ms, F&& launches) {
    K2R_HIP(hipEventRecord(e->ev0, e->stream));
    K2R_TRY(launches());
    K2R_HIP(hipEventRecord(e->ev1, e->stream));
    K2R_HIP(hipStreamSynchronize(e->stream));
    if (ms) K2R_HIP(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return DCDF_OK;
}

extern "C" int dcdf_encoder_create(const dcdf_tile_desc* tiles, size_t n, int k, size_t out_cap_per_tile,
                                   dcdf_encoder** enc_out) {
    if (!tiles || !enc_out || n == 0 || n > 0x7fffffffu) return DCDF_ERR_BAD_ARG;
    Runtime& rt = Runtime::get();
    if (!rt.ok) return DCDF_ERR_NO_DEVICE;
    std::unique_ptr<dcdf_encoder> e(new (std::nothrow) dcdf_encoder());
    if (!e) return DCDF_ERR_NOMEM;
    const SessionKnobs knobs = read_knobs();
    e->desc.assign(tiles, tiles + n);
    e->results.resize(n);
    e->plan = plan_session(tiles, n, k, out_cap_per_tile, rt.cus, knobs, encode_blocks_per_cu, encode_list_words);
    const SessionPlan& p = e->plan;
    K2R_HIP(StreamPool::get().take(false, &e->stream));
    K2R_HIP(hipEventCreate(&e->ev0));
    K2R_HIP(hipEventCreate(&e->ev1));
    K2R_HIP(e->d_out.alloc_pooled(p.out_total));
    K2R_HIP(e->d_minmax.alloc(p.minmax_total * 8));
    K2R_HIP(e->d_args.alloc(p.items.size() * sizeof(TileArgs)));
    K2R_HIP(e->d_results.alloc(p.items.size() * sizeof(TileResult)));
    if (!p.split.empty()) {
        K2R_HIP(e->d_out_b.alloc_pooled(p.parts_total));
        K2R_HIP(e->d_shared.alloc_pooled(p.shared_total));
        K2R_HIP(e->d_flags.alloc(p.flags * 16));
        K2R_TRY(upload_part_tables(e.get()));
    }
    K2R_HIP(e->d_order.alloc(std::max<size_t>(p.order_total, 1) * 4));
    K2R_HIP(e->d_queue.alloc(std::max<size_t>(p.classes.size(), 1) * 4));
    K2R_HIP(e->d_lists.alloc_pooled(std::max<size_t>(p.lists_total, 1) * 8));
    K2R_TRY(upload_orders(e.get()));
    e->args.resize(p.items.size());
    for (size_t q = 0; q < p.items.size(); q++) e->args[q] = tile_args(e.get(), p.items[q], knobs.stash_words);
    K2R_HIP(hipMemcpy(e->d_args.p, e->args.data(), e->args.size() * sizeof(TileArgs), hipMemcpyHostToDevice));
    *enc_out = e.release();
    return DCDF_OK;
}

extern "C" int dcdf_encoder_tile_kernel(const dcdf_encoder* e, size_t i, int32_t* log2_sidelen, int32_t* padded, int32_t* loader,
                                        uint32_t* generic_key) {
    if (!e || i >= e->desc.size()) return DCDF_ERR_BAD_ARG;
    const SessionPlan& p = e->plan;
    if (p.pre_status[i] != DCDF_OK) return p.pre_status[i];
    const int32_t ci = p.tile_class[i];
    if (log2_sidelen) *log2_sidelen = ci < 0 ? -1 : (int32_t)p.classes[ci].key.log2s;
    if (padded) *padded = ci < 0 ? -1 : (int32_t)p.classes[ci].key.padded;
    if (loader) *loader = ci < 0 ? -1 : (int32_t)p.classes[ci].key.vec;
    if (generic_key) *generic_key = p.tile_gkey[i];
    return DCDF_OK;
}

static int run_classes(dcdf_encoder* e, const std::vector<std::vector<uint32_t>>* subset, float* kernel_ms) {
    // subset == nullptr: all tiles of every class (order already on the device)
    const SessionPlan& p = e->plan;
    const bool stitch = !subset && !p.split.empty();
    K2R_HIP(hipMemsetAsync(e->d_queue.p, 0, e->d_queue.bytes, e->stream));
    if (stitch) K2R_HIP(hipMemsetAsync(e->d_flags.p, 0, e->d_flags.bytes, e->stream));
    return timed(e, kernel_ms, [&]() -> int {
        for (size_t ci = 0; ci < p.classes.size(); ci++) {
            uint32_t nt = (uint32_t)p.class_items[ci].size();
            if (subset) {
                nt = (uint32_t)(*subset)[ci].size();
                if (nt == 0) continue;
                K2R_HIP(hipMemcpyAsync(e->d_order.as<uint32_t>() + p.order_off[ci], (*subset)[ci].data(), nt * 4ull,
                                       hipMemcpyHostToDevice, e->stream));
            }
            EncodeLaunch L{};
            L.tiles = e->d_args.as<TileArgs>();
            L.results = e->d_results.as<TileResult>();
            L.order = e->d_order.as<uint32_t>() + p.order_off[ci];
            L.n = nt;
            L.queue = e->d_queue.as<uint32_t>() + ci;
            L.lists = e->d_lists.as<uint64_t>() + p.lists_off[ci];
            L.grid = std::min(p.grid[ci], std::max(1u, nt));
            K2R_HIP(launch_encode(p.classes[ci].key, L, e->stream));
        }
        if (stitch) {  // check and account the speculative parts (inside the timed region); bytes: materialize()
            hipLaunchKernelGGL(k2r::k_stitch<false>, dim3((uint32_t)p.split.size()), dim3(1024), 0, e->stream, e->d_part_first.as<uint32_t>(),
                               e->d_part_items.as<uint32_t>(), e->d_args.as<TileArgs>(), e->d_results.as<TileResult>());
            e->spliced = false;
        }
        return DCDF_OK;
    });
}

// The universal kernel over `tiles` (all of one (k, H)); tiles whose slot is too small are re-run into exact-size slots.
static int run_generic(dcdf_encoder* e, uint32_t key, const std::vector<uint32_t>& tiles, float* ms_acc) {
    if (tiles.empty()) return DCDF_OK;
    Runtime& rt = Runtime::get();
    const uint32_t k = key >> 8, H = key & 0xffu;
    const uint64_t per_wg = (generic_scratch_bytes(k, H) + 255) & ~255ull;
    const uint64_t budget = 8ull << 30;
    std::vector<uint32_t> todo(tiles);
    for (int pass = 0; pass < 2 && !todo.empty(); pass++) {
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)todo.size(), (uint64_t)rt.cus, budget / per_wg}));
        DevBuf d_scratch, d_order, d_queue;
        K2R_HIP(d_scratch.alloc((size_t)grid * per_wg));
        K2R_HIP(d_order.alloc(todo.size() * 4));
        K2R_HIP(d_queue.alloc(4));
        K2R_HIP(hipMemcpyAsync(d_order.p, todo.data(), todo.size() * 4, hipMemcpyHostToDevice, e->stream));
        K2R_HIP(hipMemsetAsync(d_queue.p, 0, 4, e->stream));
        EncodeLaunch L{};
        L.tiles = e->d_args.as<TileArgs>();
        L.results = e->d_results.as<TileResult>();
        L.order = d_order.as<uint32_t>();
        L.n = (uint32_t)todo.size();
        L.queue = d_queue.as<uint32_t>();
        L.lists = nullptr;
        L.grid = grid;
        float ms = 0.f;
        K2R_TRY(timed(e, &ms, [&]() -> int {
            K2R_HIP(launch_encode_generic(L, d_scratch.as<uint8_t>(), per_wg, k, H, e->stream));
            return DCDF_OK;
        }));
        if (ms_acc) *ms_acc += ms;
        K2R_TRY(download_results(e));
        std::vector<uint32_t> again;
        for (uint32_t ti : todo)
            if (e->results[ti].status == ST_OUT_CAPACITY && pass == 0) {  // res.len = the bytes it needs
                K2R_TRY(own_slot(e, ti, (e->results[ti].len + 255) & ~255ull));
                K2R_TRY(upload_tile(e, ti));
                again.push_back(ti);
            }
        todo.swap(again);
    }
    return DCDF_OK;
}

extern "C" int dcdf_encoder_run(dcdf_encoder* e, float* kernel_ms) {
    if (!e) return DCDF_ERR_BAD_ARG;
    const size_t n = e->desc.size();
    K2R_TRY(run_classes(e, nullptr, kernel_ms));
    K2R_TRY(download_results(e));
    e->splice = splice_tables(e->plan, e->results.data());
    if (std::getenv("K2R_PROFILE_PRINT")) print_profile(e->results.data(), n);
    for (size_t i = 0; i < n; i++)
        if (e->results[i].status == ST_INTERNAL) {
            const uint32_t* d = e->results[i].dbg;
            std::fprintf(stderr, "dcdf_k2r: internal guard tripped on tile %zu: guard bitmask=0x%08x (bit = kGuard* in k2r_encode.h)\n",
                         i, d[0]);
        }
    // Tiles whose slot was too small, tiles whose speculative parts did not splice: encoded again, whole (plan_retry; rare, not
    // timed) -- twice, for a tile that turns out too big for its slot only once it is whole.
    for (int pass = 0; pass < 2; pass++) {
        const Retry r = plan_retry(e->plan, e->desc.data(), e->results.data());
        if (r.tiles.empty()) break;
        for (size_t q = 0; q < r.tiles.size(); q++) {
            const uint32_t ti = r.tiles[q];
            if (r.own_cap[q]) K2R_TRY(own_slot(e, ti, r.own_cap[q]));
            e->args[ti].inst_end = 0;
            e->args[ti].shared_flag = nullptr;
            e->args[ti].shared_cmp = nullptr;
            K2R_TRY(upload_tile(e, ti));
        }
        K2R_TRY(run_classes(e, &r.again, nullptr));
        K2R_TRY(download_results(e));
        if (r.unsplit) {
            drop_parts(e->plan);
            if (!e->plan.split.empty()) K2R_TRY(upload_part_tables(e));
        }
        K2R_TRY(upload_orders(e));  // the full order lists again, for a later run()
    }
    // The universal kernel: tiles outside the fused kernel's shapes, then the tiles the fused kernel declined at run time
    // (declined_groups) -- same slot, retried with an exact-size one if need be.
    float gen_ms = 0.f;
    for (const auto& g : e->plan.generic_groups) K2R_TRY(run_generic(e, g.key, g.tiles, &gen_ms));
    for (const auto& g : declined_groups(e->plan, e->results.data())) K2R_TRY(run_generic(e, g.key, g.tiles, &gen_ms));
    if (kernel_ms) *kernel_ms += gen_ms;
    return DCDF_OK;
}

int k2r::materialize(dcdf_encoder* e) {
    if (e->spliced || e->splice.items.empty()) {
        e->spliced = true;
        return DCDF_OK;
    }
    const PartTables& t = e->splice;
    DevBuf d_first, d_items;
    K2R_HIP(d_first.alloc(t.first.size() * 4));
    K2R_HIP(d_items.alloc(t.items.size() * 4));
    K2R_HIP(hipMemcpyAsync(d_first.p, t.first.data(), t.first.size() * 4, hipMemcpyHostToDevice, e->stream));
    K2R_HIP(hipMemcpyAsync(d_items.p, t.items.data(), t.items.size() * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k2r::k_stitch<true>, dim3((uint32_t)t.first.size() - 1), dim3(1024), 0, e->stream, d_first.as<uint32_t>(),
                       d_items.as<uint32_t>(), e->d_args.as<TileArgs>(), e->d_results.as<TileResult>());
    K2R_HIP(hipGetLastError());
    K2R_HIP(hipStreamSynchronize(e->stream));
    e->spliced = true;
    return DCDF_OK;
}

extern "C" int dcdf_encoder_result(dcdf_encoder* e, size_t i, int32_t* status, uint64_t* len, uint32_t* snapshots,
                                   uint32_t* logs, const uint8_t** device_bytes) {
    if (!e || i >= e->desc.size()) return DCDF_ERR_BAD_ARG;
    if (device_bytes) K2R_TRY(materialize(e));
    const int32_t pre = e->plan.pre_status[i];
    const TileResult& r = e->results[i];
    const int st = pre == DCDF_OK ? map_status(r.status) : pre;
    if (status) *status = st;
    if (len) *len = st == DCDF_OK ? r.len : 0;
    if (snapshots) *snapshots = st == DCDF_OK ? r.snapshots : 0;
    if (logs) *logs = st == DCDF_OK ? r.logs : 0;
    if (device_bytes) *device_bytes = st == DCDF_OK ? e->args[i].out : nullptr;
    return DCDF_OK;
}

extern "C" int dcdf_encoder_fetch(dcdf_encoder* e, size_t i, uint8_t* dst, size_t cap) {
    if (!e || i >= e->desc.size() || !dst) return DCDF_ERR_BAD_ARG;
    if (e->plan.pre_status[i] != DCDF_OK) return e->plan.pre_status[i];
    const TileResult& r = e->results[i];
    if (r.status != ST_OK) return map_status(r.status);
    if (cap < r.len) return DCDF_ERR_CAPACITY;
    K2R_TRY(materialize(e));
    K2R_HIP(hipMemcpy(dst, e->args[i].out, r.len, hipMemcpyDeviceToHost));
    return DCDF_OK;
}

namespace k2r {
hipError_t launch_object_sha256(const TileArgs* tiles, const TileResult* results, uint32_t n, uint8_t* digests, hipStream_t stream);
}

extern "C" int dcdf_encoder_object_sha256(dcdf_encoder* e, uint8_t* digests, float* kernel_ms) {
    if (!e || !digests) return DCDF_ERR_BAD_ARG;
    K2R_TRY(materialize(e));
    const size_t n = e->desc.size();
    // the statuses the kernel may trust: tiles rejected on the host never reached the device
    std::vector<TileResult> res(e->results);
    for (size_t i = 0; i < n; i++)
        if (e->plan.pre_status[i] != DCDF_OK) {
            res[i].status = ST_BAD_ARG;
            res[i].len = 0;
        }
    DevBuf d_res, d_dig;
    K2R_HIP(d_res.alloc(n * sizeof(TileResult)));
    K2R_HIP(d_dig.alloc(n * 32));
    K2R_HIP(hipMemcpy(d_res.p, res.data(), n * sizeof(TileResult), hipMemcpyHostToDevice));
    K2R_TRY(timed(e, kernel_ms, [&]() -> int {
        K2R_HIP(launch_object_sha256(e->d_args.as<TileArgs>(), d_res.as<TileResult>(), (uint32_t)n, d_dig.as<uint8_t>(), e->stream));
        return DCDF_OK;
    }));
    K2R_HIP(hipMemcpy(digests, d_dig.p, n * 32, hipMemcpyDeviceToHost));
    return DCDF_OK;
}

// ---- host-side gather of the encoded buffers ("{offsets[], bytes[]} per GPU plus the per-(chunk,instant)
// (min,max) pairs") ------------------------------------------------------------------------------------
// The tiles' slots are packed on the device (16-byte aligned starts, 16-byte vector copies) and come back in ONE copy.
namespace k2r {
struct PackItem {
    const uint8_t* src;
    uint64_t len;      // bytes
    uint64_t dst_off;  // multiple of 16
};
__global__ void __launch_bounds__(256) k_pack(const PackItem* __restrict__ items, uint32_t n, uint8_t* __restrict__ dst) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const PackItem it = items[i];
        const uint4* s = (const uint4*)it.src;  // slots are 256-byte aligned and at least len rounded up to 256 long
        uint4* d = (uint4*)(dst + it.dst_off);
        const uint64_t nv = (it.len + 15) / 16;
        for (uint64_t v = threadIdx.x; v < nv; v += blockDim.x) d[v] = s[v];
    }
}
}  // namespace k2r

extern "C" int dcdf_encoder_gather_size(dcdf_encoder* e, uint64_t* packed_bytes, uint64_t* minmax_words) {
    if (!e || !packed_bytes) return DCDF_ERR_BAD_ARG;
    uint64_t tot = 0;
    for (size_t i = 0; i < e->desc.size(); i++)
        if (tile_ok(e, i)) tot += (e->results[i].len + 15) & ~15ull;
    *packed_bytes = tot;
    if (minmax_words) *minmax_words = e->plan.minmax_total;
    return DCDF_OK;
}

extern "C" int dcdf_encoder_gather(dcdf_encoder* e, uint8_t* dst, size_t cap, uint64_t* offsets, uint64_t* lens, int64_t* minmax) {
    if (!e || !dst || !offsets || !lens) return DCDF_ERR_BAD_ARG;
    K2R_TRY(materialize(e));
    const size_t n = e->desc.size();
    std::vector<PackItem> items;
    uint64_t tot = 0;
    for (size_t i = 0; i < n; i++) {
        const bool ok = tile_ok(e, i);
        offsets[i] = tot;
        lens[i] = ok ? e->results[i].len : 0;
        if (!ok || lens[i] == 0) continue;
        items.push_back(PackItem{e->args[i].out, lens[i], tot});
        tot += (lens[i] + 15) & ~15ull;
    }
    if (tot > cap) return DCDF_ERR_CAPACITY;
    if (!items.empty()) {
        // on a stream of its own: the gather only reads what a finished run left behind, so it may overlap other readers of the
        // session (the superchunk assembly hashes the objects on the session's stream meanwhile)
        struct OwnStream {
            hipStream_t s = nullptr;
            ~OwnStream() {
                if (s) StreamPool::get().give(true, s);
            }
        } own;
        K2R_HIP(StreamPool::get().take(true, &own.s));
        DevBuf d_items, d_packed;
        struct Settle {  // (declared behind the buffers: the stream is idle before an early return hands them back to the pool)
            hipStream_t s;
            ~Settle() { (void)hipStreamSynchronize(s); }
        } settle{own.s};
        K2R_HIP(d_items.alloc(items.size() * sizeof(PackItem)));
        K2R_HIP(d_packed.alloc_pooled(tot));
        K2R_HIP(hipMemcpyAsync(d_items.p, items.data(), items.size() * sizeof(PackItem), hipMemcpyHostToDevice, own.s));
        const uint32_t grid = (uint32_t)std::min<size_t>(items.size(), 8192);
        hipLaunchKernelGGL(k_pack, dim3(grid), dim3(256), 0, own.s, d_items.as<PackItem>(), (uint32_t)items.size(),
                           d_packed.as<uint8_t>());
        K2R_HIP(hipGetLastError());
        K2R_HIP(hipMemcpyAsync(dst, d_packed.p, tot, hipMemcpyDeviceToHost, own.s));
        K2R_HIP(hipStreamSynchronize(own.s));
    }
    if (minmax && e->plan.minmax_total) K2R_HIP(hipMemcpy(minmax, e->d_minmax.p, e->plan.minmax_total * 8, hipMemcpyDeviceToHost));
    return DCDF_OK;
}

extern "C" uint64_t dcdf_encoder_total_bytes(dcdf_encoder* e) {
    uint64_t s = 0;
    if (!e) return 0;
    for (size_t i = 0; i < e->desc.size(); i++)
        if (tile_ok(e, i)) s += e->results[i].len;
    return s;
}

extern "C" void dcdf_encoder_destroy(dcdf_encoder* e) { delete e; }
