// runtime.hip — the process-level plumbing under every entry point: roctx ranges, the error string, the cache of released
// device blocks, the staged transfers between caller memory and the device, and the entries that need no handle.
#include <dlfcn.h>
#include <pthread.h>
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

#include "bsn_internal.hpp"

namespace bsn {

// ---- roctx (optional) ------------------------------------------------------------------------------------------
namespace {
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (!getenv("BSN_ROCTX")) return;
    void *h = nullptr;
    for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return;
    push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
Roctx &roctx() {
  static Roctx r;
  return r;
}
}  // namespace
void roctx_push(const char *name) {
  if (roctx().push) roctx().push(name);
}
void roctx_pop() {
  if (roctx().pop) roctx().pop();
}

static thread_local std::string g_err;
void set_error(const char *msg) { g_err = msg ? msg : ""; }
void fail(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw Error(buf);
}

void require_gpu() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    fail("no HIP device available: libbigsnpr_hip has no CPU fallback (%s)",
         e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
}

// ---- cache of released device blocks (bsn_internal.hpp) ---------------------------------
namespace {
struct DevCache {
  std::mutex mu;
  std::multimap<size_t, void *> free_blocks[16];  // per device, keyed by block size
  size_t held[16] = {0};
};
DevCache &dev_cache() {
  static DevCache *c = new DevCache();  // never destroyed: blocks may be released during process exit
  return *c;
}
// sizes are rounded to 2^k or 1.5 * 2^k (>= 4 KiB) so that a repeated call finds its blocks again
size_t size_class(size_t bytes) {
  size_t c = 4096;
  while (c < bytes) {
    if (c + c / 2 >= bytes) return c + c / 2;
    c *= 2;
  }
  return c;
}
}  // namespace

void *dev_alloc(size_t bytes, size_t *granted, int *device) {
  if (bytes == 0) bytes = 1;
  int dev = 0;
  BSN_HIP(hipGetDevice(&dev));
  *device = dev;
  const bool cached = bytes <= kDevCacheMaxBlock && dev < 16;
  const size_t want = cached ? size_class(bytes) : bytes;
  if (cached) {
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.free_blocks[dev].find(want);
    if (it != c.free_blocks[dev].end()) {
      void *p = it->second;
      c.free_blocks[dev].erase(it);
      c.held[dev] -= want;
      *granted = want;
      return p;
    }
  }
  static const bool trace = getenv("BSN_ALLOC_TRACE") != nullptr;  // every real allocation on stderr
  void *p = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(&p, want);
  if (trace)
    std::fprintf(stderr, "[bsn alloc] hipMalloc %zu bytes (asked %zu): %.2f ms\n", want, bytes,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  if (e == hipErrorOutOfMemory) {  // give the cached blocks back and try once more
    (void)hipGetLastError();
    dev_cache_flush();
    e = hipMalloc(&p, want);
  }
  if (e != hipSuccess) fail("HIP error %s allocating %zu bytes of device memory", hipGetErrorString(e), want);
  *granted = want;
  return p;
}

void dev_release(void *p, size_t granted, int dev) {
  if (!p) return;
  DevCache &c = dev_cache();
  if (granted <= kDevCacheMaxBlock && dev >= 0 && dev < 16 && size_class(granted) == granted) {
    // hipFree's ordering: nothing on the device still uses the block once it can be handed out again
    int cur = dev;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    (void)hipDeviceSynchronize();
    if (cur != dev) (void)hipSetDevice(cur);
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.held[dev] + granted <= kDevCacheMaxTotal) {
      c.free_blocks[dev].emplace(granted, p);
      c.held[dev] += granted;
      return;
    }
  }
  static const bool trace = getenv("BSN_ALLOC_TRACE") != nullptr;
  if (trace) std::fprintf(stderr, "[bsn alloc] hipFree %zu bytes\n", granted);
  (void)hipFree(p);
}

size_t dev_cache_held() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
  DevCache &c = dev_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  return c.held[dev];
}

void dev_cache_flush() {
  DevCache &c = dev_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  for (int d = 0; d < 16; d++) {
    for (auto &kv : c.free_blocks[d]) (void)hipFree(kv.second);
    c.free_blocks[d].clear();
    c.held[d] = 0;
  }
}

constexpr size_t kStagePiece = 32u << 20;

void stage_init(bsn_bed *b) {
  for (int i = 0; i < 2; i++) {
    if (!b->h_stage[i]) BSN_HIP(hipHostMalloc((void **)&b->h_stage[i], kStagePiece, hipHostMallocDefault));
    if (!b->ev_stage[i]) BSN_HIP(hipEventCreateWithFlags(&b->ev_stage[i], hipEventDisableTiming));
  }
}

// Helper threads that live as long as the process (created on first use, re-created in a forked child) take their
// share of a host copy of 256 KB or more: the three m-vectors of a one-shot product at BASELINE config 2 — x, centre,
// scale, 1.6 MB each — cost 0.12 ms apiece through one core, a third of the call's time outside its streaming kernel;
// threads created per copy (round 2's way for pieces of 8 MB and more) cost more than they save at this size.  A
// helper that has just finished a share polls for the next one for some tens of microseconds before it goes to
// sleep: the copies of one call follow each other within that time, so only the first pays a wake-up.
namespace {
struct CopyJob {
  void *dst = nullptr;
  const void *src = nullptr;
  size_t len = 0;
};
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#else
  std::this_thread::yield();
#endif
}
struct CopyPool {
  static constexpr int kMaxHelpers = 6;
  int nh = 2;
  std::mutex mu;
  std::condition_variable cv_go;
  CopyJob job[kMaxHelpers];
  std::atomic<unsigned long long> seq{0};
  std::atomic<int> pending{0}, sleepers{0};
  pid_t owner = 0;
  void start() {
    owner = getpid();
    cpu_set_t set;
    int cpus = (int)std::thread::hardware_concurrency();
    if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = std::min(cpus > 0 ? cpus : 1, CPU_COUNT(&set));
    nh = std::max(1, std::min(kMaxHelpers, cpus / 2 - 1));
    if (const char *e = getenv("BSN_COPY_THREADS")) nh = std::max(1, std::min(kMaxHelpers, atoi(e) - 1));
    for (int h = 0; h < nh; h++)
      std::thread([this, h] {
        unsigned long long seen = 0;
        for (;;) {
          int spins = 0;
          while (seq.load(std::memory_order_acquire) == seen) {
            if (++spins < 4000) {
              cpu_relax();
              continue;
            }
            std::unique_lock<std::mutex> lk(mu);
            sleepers.fetch_add(1);
            cv_go.wait(lk, [&] { return seq.load() != seen; });
            sleepers.fetch_sub(1);
          }
          seen = seq.load(std::memory_order_acquire);   // (the caller waits for every share before the next copy)
          const CopyJob j = job[h];
          if (j.len) std::memcpy(j.dst, j.src, j.len);
          pending.fetch_sub(1, std::memory_order_release);
        }
      }).detach();
  }
  void copy(void *dst, const void *src, size_t len) {
    const size_t part = (len / (size_t)(nh + 1) + 63) & ~(size_t)63;
    for (int h = 0; h < nh; h++) {
      const size_t lo = part * (size_t)(h + 1), hi = h + 1 == nh ? len : std::min(len, lo + part);
      job[h] = lo < hi ? CopyJob{(uint8_t *)dst + lo, (const uint8_t *)src + lo, hi - lo} : CopyJob{};
    }
    pending.store(nh, std::memory_order_relaxed);
    seq.fetch_add(1);
    if (sleepers.load() > 0) {
      { std::lock_guard<std::mutex> lk(mu); }
      cv_go.notify_all();
    }
    std::memcpy(dst, src, std::min(part, len));
    while (pending.load(std::memory_order_acquire) != 0) cpu_relax();
  }
};
CopyPool *g_pool = nullptr;
// one copy at a time goes through the pool (calls on different handles may be concurrent: the others copy on their own
// thread instead of queueing behind it).  A raw pointer, so that the child of a fork can start from a fresh mutex: the
// parent's may have been held by a thread that does not exist in the child.
std::mutex *g_pool_mu = new std::mutex();
void pool_atfork_child() {
  g_pool_mu = new std::mutex();   // (the parent's mutex and pool object are abandoned in the child, not freed)
  g_pool = nullptr;
}
const int g_pool_atfork = pthread_atfork(nullptr, nullptr, pool_atfork_child);
}  // namespace

// host copy between caller memory and a staging buffer
static void host_copy(void *dst, const void *src, size_t len) {
  static const bool pool_off = [] {
    const char *e = getenv("BSN_COPY_THREADS");  // 1: every copy on the calling thread
    return e && atoi(e) <= 1;
  }();
  if (len < (256u << 10) || pool_off) {
    std::memcpy(dst, src, len);
    return;
  }
  std::unique_lock<std::mutex> lk(*g_pool_mu, std::try_to_lock);
  if (!lk.owns_lock()) {   // another thread's copy is in the pool: do not queue behind it
    std::memcpy(dst, src, len);
    return;
  }
  if (!g_pool || g_pool->owner != getpid()) {   // first use, or a forked child (threads do not survive a fork)
    g_pool = new CopyPool();
    g_pool->start();
  }
  g_pool->copy(dst, src, len);
}

// Host -> device through the two pinned staging buffers, ordered on the handle's stream.  Returns as
// soon as the caller's memory has been read (the last pieces may still be on their way: whatever uses
// d_dst is queued behind them on the same stream).
void copy_h2d(bsn_bed *b, void *d_dst, const void *src, size_t bytes, hipStream_t stream) {
  if (!stream) stream = b->stream;
  stage_init(b);
  for (size_t off = 0; off < bytes; off += kStagePiece) {
    const size_t len = std::min(kStagePiece, bytes - off);
    const int s = (int)(b->stage_next++ & 1);
    if (b->stage_busy[s]) BSN_HIP(hipEventSynchronize(b->ev_stage[s]));  // its previous piece has left the buffer
    host_copy(b->h_stage[s], (const uint8_t *)src + off, len);
    BSN_HIP(hipMemcpyAsync((uint8_t *)d_dst + off, b->h_stage[s], len, hipMemcpyHostToDevice, stream));
    BSN_HIP(hipEventRecord(b->ev_stage[s], stream));
    b->stage_busy[s] = true;
  }
}

// the handle's second stream: uploads that may run beside the kernels of the main one (op_cprod's centre / scale)
hipStream_t upload_stream(bsn_bed *b) {
  if (!b->stream_up) {
    BSN_HIP(hipStreamCreateWithFlags(&b->stream_up, hipStreamNonBlocking));
    BSN_HIP(hipEventCreateWithFlags(&b->ev_up, hipEventDisableTiming));
  }
  return b->stream_up;
}

// true when the runtime knows `p` as page-locked host memory (bsn_host_alloc, or registered by the
// caller): the DMA engines can reach it directly, no staging
bool host_is_pinned(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();   // an ordinary pointer is reported as an error: not one
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// Device -> host; complete when it returns.
void copy_d2h(bsn_bed *b, void *dst, const void *d_src, size_t bytes) {
  if (bytes >= (1u << 20) && host_is_pinned(dst)) {   // page-locked destination: one DMA, no host copy
    BSN_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, b->stream));
    BSN_HIP(hipStreamSynchronize(b->stream));
    return;
  }
  stage_init(b);
  if (b->stream_up)   // an upload on the second stream may still be reading a staging buffer
    for (int i = 0; i < 2; i++)
      if (b->stage_busy[i]) BSN_HIP(hipEventSynchronize(b->ev_stage[i]));
  const size_t npiece = (bytes + kStagePiece - 1) / kStagePiece;
  for (size_t k = 0; k <= npiece; k++) {
    if (k < npiece) {  // launch piece k (stream order puts it behind any upload still reading the buffer)
      const size_t off = k * kStagePiece, len = std::min(kStagePiece, bytes - off);
      BSN_HIP(hipMemcpyAsync(b->h_stage[k & 1], (const uint8_t *)d_src + off, len, hipMemcpyDeviceToHost, b->stream));
      BSN_HIP(hipEventRecord(b->ev_stage[k & 1], b->stream));
    }
    if (k >= 1) {  // drain piece k - 1 while piece k is on its way
      const size_t off = (k - 1) * kStagePiece, len = std::min(kStagePiece, bytes - off);
      BSN_HIP(hipEventSynchronize(b->ev_stage[(k - 1) & 1]));
      host_copy((uint8_t *)dst + off, b->h_stage[(k - 1) & 1], len);
    }
  }
  b->stage_busy[0] = b->stage_busy[1] = false;  // every event recorded so far has completed
}

}  // namespace bsn

using namespace bsn;

extern "C" {

const char *bsn_last_error(void) { return g_err.c_str(); }
int bsn_version(void) { return 100; }

int bsn_device_count(int *count) {
  return guarded([&] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
  });
}

int bsn_set_device(int device) {
  return guarded([&] {
    require_gpu();
    BSN_HIP(hipSetDevice(device));
  });
}

// ---- helpers ---------------------------------------------------------------------------
int bsn_malloc(void **d_ptr, int64_t bytes) {
  return guarded([&] {
    require_gpu();
    BSN_HIP(hipMalloc(d_ptr, (size_t)bytes));
  });
}
int bsn_free(void *d_ptr) {
  return guarded([&] { BSN_HIP(hipFree(d_ptr)); });
}
int bsn_host_alloc(void **h_ptr, int64_t bytes) {
  return guarded([&] {
    require_gpu();
    BSN_HIP(hipHostMalloc(h_ptr, (size_t)bytes, hipHostMallocDefault));
  });
}
int bsn_host_free(void *h_ptr) {
  return guarded([&] { BSN_HIP(hipHostFree(h_ptr)); });
}
int bsn_memcpy_h2d(void *d_dst, const void *src, int64_t bytes) {
  return guarded([&] { BSN_HIP(hipMemcpy(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice)); });
}
int bsn_memcpy_d2h(void *dst, const void *d_src, int64_t bytes) {
  return guarded([&] { BSN_HIP(hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost)); });
}
int bsn_device_sync(void) {
  return guarded([&] { BSN_HIP(hipDeviceSynchronize()); });
}

}  // extern "C"
