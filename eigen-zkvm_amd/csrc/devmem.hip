// Device memory of libzkgpu: the caching allocator, the registry of streams the library works on, the binding of host threads
// to the GPU of zk_init, the scope of one C-ABI call and the per-thread error string.  Every device block of the library is
// taken and given back here (zk_internal.h: pool_*, DevBuf, DevConst).
#include "zk_internal.h"
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <vector>
namespace zk {

static thread_local std::string t_err;
void set_error(const std::string& msg) { t_err = msg; }
const char* last_error() { return t_err.c_str(); }

// ---- caching device allocator -------------------------------------------------------------------
namespace {
// An event recorded when blocks were freed; shared by all blocks freed in one burst (pool_defer_*), recycled by the last of them
struct Ev { hipEvent_t e = nullptr; int refs = 0; };
struct Block { size_t bytes = 0; std::vector<Ev*> pending; };
std::mutex g_pool_mu;
std::multimap<size_t, void*> g_pool_free;   // size -> idle block
std::map<void*, Block> g_pool_blocks;       // every block handed out by pool_alloc
std::vector<hipStream_t> g_streams{nullptr};  // streams the library has been asked to work on
std::vector<hipEvent_t> g_event_cache;
thread_local hipStream_t t_stream = nullptr;
thread_local std::vector<hipStream_t> t_streams;   // non-null streams this host thread has issued on
thread_local int t_depth = 0;                      // C-ABI calls in progress on this thread (the prover calls entry points itself)
thread_local bool t_defer = false;                 // pool_defer_begin(): frees are collected ...
thread_local std::vector<void*> t_deferred;        // ... here, and stamped with ONE set of events by pool_defer_flush()
int g_reserving = 0;                               // pool_reserve_async helpers that may hold blocks (g_pool_mu held)
std::condition_variable g_reserve_cv;              // ... signalled when one of them has parked its blocks
thread_local bool t_reserving = false;             // this thread is such a helper: it never waits for the others
void ev_release(Ev* v) { if (--v->refs == 0) { g_event_cache.push_back(v->e); delete v; } }   // g_pool_mu held

hipEvent_t event_get() {                     // g_pool_mu held; never throws (DevBuf destructors end up here): nullptr = no event to be had
    if (!g_event_cache.empty()) { hipEvent_t e = g_event_cache.back(); g_event_cache.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return e;
}
}
hipStream_t cur_stream() { return t_stream; }
// The GPU of the process (zk_init).  HIP's current device is a property of the host thread and every new thread starts on device 0,
// so a prover thread of rank k > 0 would otherwise allocate and launch on GPU 0: each thread is bound on its first call.
static std::atomic<int> g_device{-1};          // -1: zk_init was never called, threads are left as the caller set them up
// zk_init's device overrides whatever the caller (torch.cuda.set_device, another library) made current on this thread in the
// meantime: pooled blocks, constant tables and code modules all belong to device d, so every outermost call re-checks the thread's
// actual device (hipGetDevice is a thread-local read) instead of trusting a flag cached at the first call.
void set_device(int d) { g_device.store(d, std::memory_order_relaxed); }
void bind_device() noexcept {
    const int d = g_device.load(std::memory_order_relaxed);
    if (d < 0) return;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == d) return;
    if (hipSetDevice(d) != hipSuccess) (void)hipGetLastError();   // the work that follows reports its own error
}
CallScope::CallScope() : saved(t_stream) { if (t_depth++ == 0) { t_stream = nullptr; bind_device(); } }   // a call from outside starts on the null stream,
// one made by the prover inherits the prover's.  Frees deferred during the call (pool_defer_begin) go back when the outermost call
// returns, after its locals are gone and also when it threw; calls the prover makes meanwhile (a tree's destructor) leave them collected.
CallScope::~CallScope() { if (--t_depth == 0) pool_defer_flush(); t_stream = saved; }
hipStream_t on_stream(hipStream_t st) {
    t_stream = st;
    if (st) {
        bool mine = false;
        for (hipStream_t s : t_streams) mine |= s == st;
        if (!mine) {
            t_streams.push_back(st);
            std::lock_guard<std::mutex> lk(g_pool_mu);
            bool known = false;
            for (hipStream_t s : g_streams) known |= s == st;
            if (!known) {
                // While the null stream was the only one in use, blocks went back to the pool without an event (pool_free):
                // work queued there may still be running on them, and a non-blocking stream does not wait for the null stream.
                // Drain once, at the moment a second stream appears; from here on every free records its events.
                // (under the lock on purpose: no block may be handed out between the drain and the registration)
                if (g_streams.size() == 1) (void)hipDeviceSynchronize();
                g_streams.push_back(st);
            }
        }
    }
    return st;
}
// A helper stream that lives inside one call (the MSM's sort stream): registered so that this thread's frees are stamped on it while it
// is in use, WITHOUT the one-off device drain of on_stream -- the caller guarantees that the side stream's first operation waits for an
// event recorded on the current stream after every buffer it will touch was allocated (so it is ordered behind those blocks' previous
// users), and calls forget_stream once the current stream has waited for the side stream's last event.  The thread's current stream is kept.
void on_side_stream(hipStream_t ss) {
    if (!ss) return;
    bool mine = false;
    for (hipStream_t s : t_streams) mine |= s == ss;
    if (!mine) t_streams.push_back(ss);
    std::lock_guard<std::mutex> lk(g_pool_mu);
    bool known = false;
    for (hipStream_t s : g_streams) known |= s == ss;
    if (!known) g_streams.push_back(ss);
}
namespace {
void* raw_alloc(size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {  // out of memory: drop the cache and retry once
        (void)hipGetLastError();                                      // the failed attempt must not surface at a later check
        if (!t_reserving) {                                           // blocks a reservation helper holds are about to be cached: wait for them
            std::unique_lock<std::mutex> lk(g_pool_mu);
            g_reserve_cv.wait(lk, [] { return g_reserving == 0; });
        }
        pool_trim();
        ZK_HIP(hipMalloc(&p, bytes));
    }
    return p;
}
}  // namespace
void* pool_alloc(size_t bytes, bool host_wait) {
    if (bytes == 0) bytes = 8;
    {
        std::unique_lock<std::mutex> lk(g_pool_mu);
        auto it = g_pool_free.find(bytes);
        if (it != g_pool_free.end()) {
            void* p = it->second; g_pool_free.erase(it);
            std::vector<Ev*> pending;
            pending.swap(g_pool_blocks[p].pending);                   // the block is out of the free list: nobody else sees it or its events' list
            // whoever used the block last finishes first.  The library's own buffers: the stream this thread works on waits
            // (asynchronous, under the lock).  A block that leaves the library (zk_dev_alloc: the caller may touch it from any
            // stream): the HOST waits -- with the lock released, so that other provers' allocations and frees go on meanwhile.
            if (host_wait) lk.unlock();
            for (Ev* v : pending) {
                const hipError_t rc = host_wait ? hipEventSynchronize(v->e) : hipStreamWaitEvent(t_stream, v->e, 0);
                // an event whose stream has been destroyed since (a released setup's side stream: drained before it went) reports an
                // error here; its work is done, and the error must not surface at some later hipGetLastError()
                if (rc != hipSuccess) (void)hipGetLastError();
            }
            if (host_wait) lk.lock();
            for (Ev* v : pending) ev_release(v);
            return p;
        }
    }
    void* p = raw_alloc(bytes);
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_blocks[p].bytes = bytes;
    return p;
}
// Process-lifetime constants (DevConst): from the driver like a pooled block, but never entered in g_pool_blocks -- the free list
// cannot recycle them and pool_trim() does not see them.
void* const_alloc(size_t bytes) { return raw_alloc(bytes ? bytes : 8); }
void const_free(void* p) noexcept { if (p && hipFree(p) != hipSuccess) (void)hipGetLastError(); }
// The blocks of `sizes` are taken on a helper thread and parked in the free list (stark_prover.hip setup_new: a proof's large buffers,
// beside the compilers and the constants' upload).  While a helper holds blocks pool_trim() cannot see them, so an allocation that
// runs out of memory meanwhile waits for the helpers before it trims (raw_alloc).  Out of memory on the helper itself: what fits
// is parked, the proof asks for the rest.
static void reserve_end() { { std::lock_guard<std::mutex> lk(g_pool_mu); --g_reserving; } g_reserve_cv.notify_all(); }
std::future<void> pool_reserve_async(std::vector<size_t> sizes) {
    int dev = 0; ZK_HIP(hipGetDevice(&dev));
    { std::lock_guard<std::mutex> lk(g_pool_mu); ++g_reserving; }       // counted from before the helper starts until its blocks are parked
    try {
        return std::async(std::launch::async, [sizes = std::move(sizes), dev] {
            struct End { ~End() { reserve_end(); } } end;
            t_reserving = true;
            if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); return; }
            std::vector<void*> blocks;
            try { for (size_t b : sizes) blocks.push_back(pool_alloc(b)); } catch (...) {}
            for (void* q : blocks) pool_free(q);
        });
    } catch (...) { reserve_end(); throw; }                           // no thread to be had
}
namespace {
// events for blocks freed now: the null stream and every stream the FREEING thread has issued on (a buffer is released by the
// thread that owns it; work another thread did on it was ordered before this thread's by whoever handed it over).  Streams of
// other threads are left alone: concurrent provers must not wait for each other.  g_pool_mu held.
std::vector<Ev*> stamp_now() {
    std::vector<Ev*> out;
    if (g_streams.size() <= 1) return out;               // a single stream in use: reuse is stream ordered (on_stream drains at the second)
    auto record = [&](hipStream_t st) {
        hipEvent_t e = event_get();
        if (!e) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return; }   // no event to be had: wait here instead
        if (hipEventRecord(e, st) == hipSuccess) out.push_back(new Ev{e, 0});
        else { (void)hipGetLastError(); g_event_cache.push_back(e); }   // a destroyed stream has nothing in flight
    };
    record(nullptr);
    for (hipStream_t st : t_streams) record(st);
    return out;
}
void release_stamped(void* p, const std::vector<Ev*>& evs) {   // g_pool_mu held
    auto it = g_pool_blocks.find(p);
    if (it == g_pool_blocks.end()) { (void)hipFree(p); return; }
    for (Ev* v : evs) { ++v->refs; it->second.pending.push_back(v); }
    g_pool_free.emplace(it->second.bytes, p);
}
}  // namespace
void pool_free(void* p) {
    if (!p) return;
    if (t_defer) { t_deferred.push_back(p); return; }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    const std::vector<Ev*> evs = stamp_now();
    release_stamped(p, evs);
    for (Ev* v : evs) if (v->refs == 0) { g_event_cache.push_back(v->e); delete v; }   // the block was not the pool's
}
// A burst of frees with no launch in between (the end of a proof: ~70 buffers and trees go at once) shares one set of events
// instead of recording two per block: pool_defer_begin() after the last launch, pool_defer_flush() once the destructors have run.
void pool_defer_begin() { t_defer = true; }
void pool_defer_flush() {
    t_defer = false;
    if (t_deferred.empty()) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    const std::vector<Ev*> evs = stamp_now();
    for (void* p : t_deferred) release_stamped(p, evs);
    for (Ev* v : evs) if (v->refs == 0) { g_event_cache.push_back(v->e); delete v; }
    t_deferred.clear();
}
// Host <-> device copies of the library's own pooled buffers: on the stream this thread is working on (the one whose
// queue was ordered behind the buffer's previous user by pool_alloc), then waited for -- a plain hipMemcpy runs on the
// null stream, which a non-blocking stream does not synchronise with.
void h2d_sync(void* d, const void* h, size_t n) {
    if (!n) return;
    ZK_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, t_stream));
    ZK_HIP(hipStreamSynchronize(t_stream));
}
void d2h_sync(void* h, const void* d, size_t n) {
    if (!n) return;
    ZK_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, t_stream));
    ZK_HIP(hipStreamSynchronize(t_stream));
}
void pool_trim() {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto& kv : g_pool_free) {
        Block& b = g_pool_blocks[kv.second];
        for (Ev* v : b.pending) { if (hipEventSynchronize(v->e) != hipSuccess) (void)hipGetLastError(); ev_release(v); }
        (void)hipFree(kv.second); g_pool_blocks.erase(kv.second);
    }
    g_pool_free.clear();
}
void forget_stream(hipStream_t st) {                                  // before hipStreamDestroy
    for (size_t i = 0; i < t_streams.size(); ++i)
        if (t_streams[i] == st) { t_streams.erase(t_streams.begin() + i); break; }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 1; i < g_streams.size(); ++i)
        if (g_streams[i] == st) { g_streams.erase(g_streams.begin() + i); break; }
}

}  // namespace zk
