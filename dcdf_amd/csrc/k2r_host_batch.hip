// k2r_host_batch.hip -- C ABI, the host-buffer path of the encode side (include/dcdf_k2r.h).  Host code only.
//
// dcdf_chunk_build_batch = upload + session + download: Chunk::build for a batch.  The pinned ring, the packing threads and
// encoder_download also serve k2r_superchunk.hip.  The session is reached through k2r_session.h only.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <sched.h>

#include "k2r_session.h"

using namespace k2r;

extern "C" void dcdf_free_encoded(dcdf_encoded* out, size_t n) {
    if (!out) return;
    for (size_t i = 0; i < n; i++) {
        std::free(out[i].bytes);
        std::free(out[i].minmax);
    }
    std::free(out);
}

// Host-side transfer machinery of the host-buffer entry point: two pinned staging buffers filled by a few packing
// threads while the previous one is in flight on the copy engine (uploads), and drained the same way (downloads).
namespace {

constexpr size_t kPinBytes = 64u << 20;
constexpr int kDownSlots = 4;                            // downloads see the two buffers as four slots ...
constexpr size_t kSlotBytes = 2 * kPinBytes / kDownSlots;  // ... of 32 MB, each with its own event

// Host threads for packing, unpacking and hashing: one and a half per CPU this process may use (they wait on page faults and on
// the copy engine as much as they compute) -- the cgroup's CPU quota where there is one, else the affinity mask -- 32 at most.
// K2R_HOST_THREADS overrides.
int host_threads() {
    static const int n = [] {
        if (const char* e = std::getenv("K2R_HOST_THREADS")) {
            const int v = std::atoi(e);
            if (v >= 1) return std::min(v, 64);
        }
        int c = 0;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) c = CPU_COUNT(&set);
        if (c <= 0) c = (int)std::thread::hardware_concurrency();
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
            long long quota = 0, period = 0;
            if (std::fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
                c = std::min<int>(c, (int)std::max<long long>(1, (quota + period - 1) / period));
            std::fclose(f);
        }
        return std::max(1, std::min(c + c / 2, 32));
    }();
    return n;
}

struct PinRing {
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t slot_ev[kDownSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool busy[2] = {false, false};
    hipStream_t stream = nullptr;
    bool ok = false;
    std::mutex mu;  // one host-buffer batch at a time uses the ring
    bool init() {
        if (ok) return true;
        for (int i = 0; i < 2; i++) {
            // page-locked if the system allows it; otherwise ordinary memory (the copies then stage inside the runtime)
            if (!buf[i] && hipHostMalloc(&buf[i], kPinBytes, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                buf[i] = std::malloc(kPinBytes);
                if (!buf[i]) return false;
            }
            if (!ev[i] && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
        }
        for (int i = 0; i < kDownSlots; i++)
            if (!slot_ev[i] && hipEventCreateWithFlags(&slot_ev[i], hipEventDisableTiming) != hipSuccess) return false;
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return false;
        ok = true;
        return true;
    }
    bool wait(int b) {
        if (busy[b] && hipEventSynchronize(ev[b]) != hipSuccess) return false;
        busy[b] = false;
        return true;
    }
    uint8_t* slot(int s) const { return (uint8_t*)buf[s / (kDownSlots / 2)] + (size_t)(s % (kDownSlots / 2)) * kSlotBytes; }
};
PinRing& pin_ring() {
    static PinRing r;
    return r;
}

// runs f(0..n) on up to host_threads() threads
template <class F>
void parallel_for(size_t n, F&& f) {
    const size_t nt = std::min<size_t>((size_t)host_threads(), n);
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    std::vector<std::thread> th;
    std::atomic<size_t> next{0};
    for (size_t t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= n) break;
                f(i);
            }
        });
    for (auto& t : th) t.join();
}

// dense copy of a (possibly strided) host tile (mmbuffer.rs:517-522 tile slices)
void pack_tile(const dcdf_tile_desc& t, uint8_t* d) {
    const size_t es = elem_size(t.dtype);
    const uint8_t* src = (const uint8_t*)t.base;
    const bool contiguous = t.stride_c == 1 && t.stride_r == (int64_t)t.cols && t.stride_t == (int64_t)t.rows * t.cols;
    if (contiguous) {
        std::memcpy(d, src, (size_t)t.instants * t.rows * t.cols * es);
        return;
    }
    for (uint32_t a = 0; a < t.instants; a++)
        for (uint32_t r = 0; r < t.rows; r++) {
            const uint8_t* row = src + ((int64_t)a * t.stride_t + (int64_t)r * t.stride_r) * (int64_t)es;
            if (t.stride_c == 1) {
                std::memcpy(d, row, (size_t)t.cols * es);
                d += (size_t)t.cols * es;
            } else {
                for (uint32_t c = 0; c < t.cols; c++, d += es) std::memcpy(d, row + (int64_t)c * t.stride_c * (int64_t)es, es);
            }
        }
}

}  // namespace

static int build_group(const dcdf_tile_desc* tiles, size_t n, int k, int mem, dcdf_encoded* out) {
    // tiles[0..n) fit the staging budget; host tiles are packed contiguously and uploaded
    std::vector<dcdf_tile_desc> dev(tiles, tiles + n);
    DevBuf stage;
    PinRing& ring = pin_ring();
    std::unique_lock<std::mutex> ring_lock(ring.mu, std::defer_lock);
    if (mem == DCDF_MEM_HOST) {
        ring_lock.lock();
        if (!ring.init()) return DCDF_ERR_NOMEM;
        uint64_t total = 0;
        std::vector<uint64_t> off(n), bytes(n, 0);
        for (size_t i = 0; i < n; i++) {
            off[i] = total;
            const dcdf_tile_desc& t = tiles[i];
            if (!desc_ok(t)) continue;
            bytes[i] = (uint64_t)t.instants * t.rows * t.cols * elem_size(t.dtype);
            total += (bytes[i] + 255) & ~255ull;
        }
        K2R_HIP(stage.alloc(total));
        // fills: runs of tiles whose staged range fits one pinned buffer (a tile larger than that goes alone, in pieces)
        size_t i = 0;
        int fill = 0;
        while (i < n) {
            if (bytes[i] == 0) {
                i++;
                continue;
            }
            const int b = fill & 1;
            if (!ring.wait(b)) return DCDF_ERR_NO_DEVICE;
            if (bytes[i] > kPinBytes) {  // oversize tile: dense temporary, then piecewise through the ring
                std::vector<uint8_t> tmp(bytes[i]);
                pack_tile(tiles[i], tmp.data());
                for (uint64_t o = 0; o < bytes[i]; o += kPinBytes) {
                    const int bb = fill & 1;
                    if (!ring.wait(bb)) return DCDF_ERR_NO_DEVICE;
                    const size_t len = (size_t)std::min<uint64_t>(kPinBytes, bytes[i] - o);
                    std::memcpy(ring.buf[bb], tmp.data() + o, len);
                    K2R_HIP(hipMemcpyAsync(stage.as<uint8_t>() + off[i] + o, ring.buf[bb], len, hipMemcpyHostToDevice, ring.stream));
                    K2R_HIP(hipEventRecord(ring.ev[bb], ring.stream));
                    ring.busy[bb] = true;
                    fill++;
                }
                i++;
                continue;
            }
            size_t j = i;
            const uint64_t base_off = off[i];
            while (j < n && (bytes[j] == 0 || off[j] + bytes[j] - base_off <= kPinBytes)) j++;
            uint8_t* pb = (uint8_t*)ring.buf[b];
            parallel_for(j - i, [&](size_t q) {
                const size_t ti = i + q;
                if (bytes[ti]) pack_tile(tiles[ti], pb + (off[ti] - base_off));
            });
            const uint64_t len = (j < n ? off[j] : total) - base_off;
            K2R_HIP(hipMemcpyAsync(stage.as<uint8_t>() + base_off, pb, std::min<uint64_t>(len, kPinBytes), hipMemcpyHostToDevice, ring.stream));
            K2R_HIP(hipEventRecord(ring.ev[b], ring.stream));
            ring.busy[b] = true;
            fill++;
            i = j;
        }
        if (!ring.wait(0) || !ring.wait(1)) return DCDF_ERR_NO_DEVICE;
        for (size_t q = 0; q < n; q++) {
            if (!bytes[q]) continue;
            const dcdf_tile_desc& t = tiles[q];
            dev[q].base = stage.as<uint8_t>() + off[q];
            dev[q].stride_c = 1;
            dev[q].stride_r = t.cols;
            dev[q].stride_t = (int64_t)t.rows * t.cols;
        }
    }
    dcdf_encoder* e = nullptr;
    int rc = dcdf_encoder_create(dev.data(), n, k, 0, &e);
    if (rc != DCDF_OK) return rc;
    std::unique_ptr<dcdf_encoder> guard(e);
    rc = dcdf_encoder_run(e, nullptr);
    if (rc != DCDF_OK) return rc;
    std::vector<int64_t> mm(e->plan.minmax_total);
    if (!mm.empty()) K2R_HIP(hipMemcpy(mm.data(), e->d_minmax.p, mm.size() * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> lens(n, 0);
    for (size_t i = 0; i < n; i++) {
        int32_t st;
        uint64_t len;
        uint32_t ns, nl;
        dcdf_encoder_result(e, i, &st, &len, &ns, &nl, nullptr);
        out[i].status = st;
        out[i].len = 0;
        out[i].bytes = nullptr;
        out[i].minmax = nullptr;
        out[i].snapshots = ns;
        out[i].logs = nl;
        {
            int32_t lg = -1, pd = -1, ld = -1;
            uint32_t gk = 0;
            out[i].kernel = 0;
            if (dcdf_encoder_tile_kernel(e, i, &lg, &pd, &ld, &gk) == DCDF_OK)
                out[i].kernel = gk ? (int32_t)gk : (int32_t)((1u << 24) | ((uint32_t)ld << 16) | ((uint32_t)pd << 8) | (uint32_t)lg);
        }
        if (st != DCDF_OK) continue;
        out[i].bytes = (uint8_t*)std::malloc(len ? len : 1);
        out[i].minmax = (int64_t*)std::malloc(16ull * tiles[i].instants);
        if (!out[i].bytes || !out[i].minmax) return DCDF_ERR_NOMEM;
        lens[i] = len;
        out[i].len = len;
        std::memcpy(out[i].minmax, mm.data() + e->plan.minmax_off[i], 16ull * tiles[i].instants);
    }
    // encoded bytes: device slots -> pinned buffer (async, one copy per tile) -> the caller's buffers (threads)
    if (ring_lock.owns_lock()) ring_lock.unlock();
    return k2r::encoder_download(e, [&](size_t i, uint64_t) { return out[i].bytes; });
}

namespace k2r {
void host_parallel_for(size_t n, const std::function<void(size_t)>& f) { parallel_for(n, f); }
int host_thread_count() { return host_threads(); }

int encoder_download(dcdf_encoder* e, const std::function<uint8_t*(size_t, uint64_t)>& dst, const std::function<void(size_t)>& landed) {
    K2R_TRY(materialize(e));
    const size_t n = e->desc.size();
    std::vector<uint64_t> lens(n, 0);
    for (size_t i = 0; i < n; i++)
        if (tile_ok(e, i)) lens[i] = e->results[i].len;
    PinRing& ring = pin_ring();
    std::lock_guard<std::mutex> ring_lock(ring.mu);
    if (!ring.init()) return DCDF_ERR_NOMEM;
    // The copy engine fills one 32 MB slot of the pinned ring after the other (one asynchronous copy per object, one event per slot);
    // worker threads take the objects of a slot as soon as its event has fired -- destination from `dst`, memcpy, `landed` (the
    // caller's hash) -- and a slot is filled again when its last object has been taken out.  Copy, unpacking and hashing of
    // different slots overlap; nothing waits for a whole buffer.
    struct Task {
        size_t tile;
        int slot;
        uint64_t off;
    };
    std::mutex mu;
    std::condition_variable cv_task, cv_slot;
    std::deque<Task> tasks;
    int outstanding[kDownSlots] = {0, 0, 0, 0};
    bool closing = false;
    std::atomic<bool> nomem{false}, hipfail{false};
    auto worker = [&] {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_task.wait(lk, [&] { return !tasks.empty() || closing; });
                if (tasks.empty()) return;
                t = tasks.front();
                tasks.pop_front();
            }
            if (hipEventSynchronize(ring.slot_ev[t.slot]) != hipSuccess) hipfail = true;
            else if (uint8_t* d = dst(t.tile, lens[t.tile])) {
                std::memcpy(d, ring.slot(t.slot) + t.off, lens[t.tile]);
                if (landed) landed(t.tile);
            } else nomem = true;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--outstanding[t.slot] == 0) cv_slot.notify_all();
            }
        }
    };
    size_t n_big = 0;
    for (size_t i = 0; i < n; i++) n_big += lens[i] != 0 && lens[i] <= kSlotBytes;
    std::vector<std::thread> pool;
    for (size_t t = 0, nt = std::min<size_t>((size_t)host_threads(), n_big); t < nt; t++) pool.emplace_back(worker);
    // Every exit leaves the ring as the next caller expects it: workers gone, no copy still landing in a pinned buffer.
    auto finish = [&](int rc) -> int {
        {
            std::lock_guard<std::mutex> lk(mu);
            closing = true;
        }
        cv_task.notify_all();
        for (auto& t : pool) t.join();
        if (rc != DCDF_OK || hipfail) (void)hipStreamSynchronize(ring.stream);
        if (rc != DCDF_OK) return rc;
        if (hipfail) return DCDF_ERR_NO_DEVICE;
        return nomem ? DCDF_ERR_NOMEM : DCDF_OK;
    };
#define K2R_HIP_Q(call)                                                 \
    do {                                                                \
        hipError_t _e = (call);                                         \
        if (_e != hipSuccess) return finish(k2r::map_hip_error(_e));    \
    } while (0)
    size_t i = 0;
    int fill = 0;
    while (i < n) {
        if (lens[i] == 0) {
            i++;
            continue;
        }
        if (lens[i] > kSlotBytes) {  // oversize result: plain copy
            uint8_t* d = dst(i, lens[i]);
            if (!d) return finish(DCDF_ERR_NOMEM);
            K2R_HIP_Q(hipMemcpy(d, e->args[i].out, lens[i], hipMemcpyDeviceToHost));
            if (landed) landed(i);
            i++;
            continue;
        }
        const int s = fill % kDownSlots;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_slot.wait(lk, [&] { return outstanding[s] == 0; });
        }
        std::vector<Task> batch;
        uint64_t used = 0;
        while (i < n && (lens[i] == 0 || (lens[i] <= kSlotBytes && used + lens[i] <= kSlotBytes))) {
            if (lens[i]) {
                K2R_HIP_Q(hipMemcpyAsync(ring.slot(s) + used, e->args[i].out, lens[i], hipMemcpyDeviceToHost, ring.stream));
                batch.push_back(Task{i, s, used});
                used += (lens[i] + 63) & ~63ull;
            }
            i++;
        }
        K2R_HIP_Q(hipEventRecord(ring.slot_ev[s], ring.stream));
        {
            std::lock_guard<std::mutex> lk(mu);
            outstanding[s] = (int)batch.size();
            for (const Task& t : batch) tasks.push_back(t);
        }
        cv_task.notify_all();
        fill++;
    }
#undef K2R_HIP_Q
    return finish(DCDF_OK);
}
}  // namespace k2r

extern "C" int dcdf_chunk_build_batch(const dcdf_tile_desc* tiles, size_t n, int k, int mem, dcdf_encoded** out) {
    if (!tiles || !out || n == 0 || (mem != DCDF_MEM_HOST && mem != DCDF_MEM_DEVICE)) return DCDF_ERR_BAD_ARG;
    if (!Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    dcdf_encoded* res = (dcdf_encoded*)std::calloc(n, sizeof(dcdf_encoded));
    if (!res) return DCDF_ERR_NOMEM;
    const uint64_t budget = 4ull << 30;  // raw bytes staged per group
    size_t i = 0;
    while (i < n) {
        uint64_t acc = 0;
        size_t j = i;
        while (j < n) {
            const uint64_t b = (uint64_t)tiles[j].instants * tiles[j].rows * tiles[j].cols * elem_size(tiles[j].dtype);
            if (j > i && acc + b > budget) break;
            acc += b;
            j++;
        }
        const int rc = build_group(tiles + i, j - i, k, mem, res + i);
        if (rc != DCDF_OK) {
            dcdf_free_encoded(res, n);
            return rc;
        }
        i = j;
    }
    *out = res;
    return DCDF_OK;
}

extern "C" int dcdf_chunk_build(const dcdf_tile_desc* tile, int k, int mem, dcdf_encoded** out) {
    return dcdf_chunk_build_batch(tile, 1, k, mem, out);
}
