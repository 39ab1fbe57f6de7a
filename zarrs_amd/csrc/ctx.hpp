// The context (one per GPU: the caching allocator and the lanes), the owners of the memory taken from
// its pools, and the per-thread call state, shared by the host translation units of libzgpu.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "internal.hpp"

// device counters in the plan's control block (u64 each, cleared per execute)
enum { CTR_ENC_BYTES = 0, CTR_ZSTD_SERIAL = 1, CTR_ZSTD_PARALLEL = 2, CTR_BLOSC_RERUN = 3, CTR_BLOSC_BLOCKS = 4,
       CTR_ITEMS = 5, CTR_ZSTD_LATENCY = 6, CTR_BZ2_BLOCKS = 7, CTR_BZ2_ROUNDS = 8,  // CTR_ITEMS and CTR_BZ2_ROUNDS are host-side
       CTR_STORE_DECODED = 9, CTR_STORE_ENCODED = 10, CTR_STORE_CARRIED = 11,  // the store path's (store.cpp), host-side
       CTR_POINT_LEAVES = 12, CTR_POINT_ROUNDS = 13,  // the read by coordinates' (points.cpp), host-side
       CTR_BLOSC_ALIASED = 14, CTR_N = 15 };  // alias entries k_zstd_plan wrote for the blosc stage (k_zstd_alias_count)
// internal ctl slots (not reported): a cached blosc layout was outgrown (the execution is re-run)
enum { CTR_BLOSC_OVF = 31, CTR_SCRATCH = 30, CTR_ZSTD_NSER = 29, CTR_ZSTD_MAXBLK = 28 };  // not reported (device-side flags / sinks)
// UnexpectedChunkDecodedSize detail of the last call's first DECODED_SIZE_MISMATCH descriptor
struct SizeDetail {
  int valid = 0;
  uint64_t desc = 0, len = 0, expected = 0;
};

#pragma GCC visibility push(hidden)  // nothing below is part of the C ABI
// The calling thread's state behind zgpu_last_error, zgpu_last_counters and zgpu_last_size_mismatch is
// thread_local in zgpu.cpp, its one definition; the other translation units reach it through these.
int set_err(int st, const std::string &m);  // sets the thread's error message; returns st
SizeDetail &size_detail();
uint64_t *call_counters();  // CTR_N counters, summed over the plans the call ran
struct HipFail {
  hipError_t e;
  const char *what;
};
#define HIPCHK(x)                                   \
  do {                                              \
    hipError_t _e = (x);                            \
    if (_e != hipSuccess) throw HipFail{_e, #x};    \
  } while (0)

// every C ABI entry point turns the exceptions into a status and the thread's error message
#define ABI_GUARD_BEGIN try {
#define ABI_GUARD_END                                                                          \
  }                                                                                            \
  catch (const ChainError &e) {                                                                \
    return set_err(e.status, e.msg);                                                           \
  }                                                                                            \
  catch (const HipFail &e) {                                                                   \
    return set_err(ZGPU_HIP_ERROR, std::string(e.what) + ": " + hipGetErrorString(e.e));       \
  }                                                                                            \
  catch (const std::exception &e) {                                                            \
    return set_err(ZGPU_INVALID_ARGUMENT, e.what());                                           \
  }

// ------------------------------------------------------------------------------------------------
// Context: one per GPU. Owns a caching device allocator (grow-only pools reused across calls so a
// steady-state decode performs no hipMalloc) and a small pool of "lanes" (a stream, two copy streams
// and an ordering event): concurrent calls on one context each take a lane and run side by side on
// the GPU (zarrs calls a codec from many rayon workers at once); a call that finds every lane busy
// waits for one. ZGPU_CTX_LANES sets the pool size (default 8: coalesced drop-in calls measured
// 10.7 -> 11.6 GiB/s going from 4 to 8, profiles/r04o_dropin_lanes_ab.txt).
// ------------------------------------------------------------------------------------------------
struct Coalescer;
void delete_coalescer(Coalescer *co);

struct Lane {
  hipStream_t stream = nullptr;              // the call's stream when the caller passes none
  hipStream_t copy[2] = {nullptr, nullptr};  // H2D / D2H streams of the pipelined host paths (lazy)
  hipStream_t out_hi = nullptr;               // high-priority stream of a coalesced batch's pack + D2H (lazy)
  hipEvent_t order_ev = nullptr;              // legacy-stream -> lane-stream ordering (pick_stream)
};

// A lane's stream. HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default), and
// kernels of different streams sharing a queue run one after the other: 8 lanes (plus their pack
// streams) on 4 queues serialised the drop-in's concurrent calls. A stream with a CU mask gets a
// hardware queue of its own; with every CU in the mask (ZGPU_LANE_QUEUES=1) it is an ordinary stream
// otherwise. HIP creates CU-masked streams as blocking streams (ordered against the legacy null stream,
// unlike the non-blocking lanes they replace), and has no flags argument for them: with
// ZGPU_LANE_QUEUES=1, work a caller queues on the null stream serialises with the lanes.
inline hipError_t lane_stream_create(hipStream_t *s, int device) {
  static const bool own = [] {
    const char *e = std::getenv("ZGPU_LANE_QUEUES");
    return e && std::atoi(e) != 0;
  }();
  if (own) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) {
      std::vector<uint32_t> mask((ncu + 31) / 32, ~0u);
      if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1;
      const hipError_t e = hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
      if (e == hipSuccess) return e;
      (void)hipGetLastError();
    }
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

struct zgpu_ctx {
  int device = 0;
  // Lifetime: zgpu_ctx_destroy drops the caller's reference; every chain, plan and cache created on
  // the context holds one more, so a context outlives the objects that use it in whatever order a
  // garbage-collected binding destroys them. The last reference frees the context (no HIP call runs
  // from a static destructor: the library has none).
  std::atomic<int64_t> refs{1};
  std::mutex mu;  // the allocator pools
  std::multimap<size_t, void *> free_dev;  // size -> ptr
  std::map<void *, size_t> live_dev;
  std::multimap<size_t, void *> free_host;
  std::map<void *, size_t> live_host;
  // lanes
  std::mutex lane_mu;
  std::condition_variable lane_cv;
  std::vector<Lane *> lanes_all, lanes_free;
  uint32_t max_lanes = 8;
  hipStream_t peer = nullptr;  // peer copies of the multi-device read (lazy)
  struct Coalescer *co = nullptr;  // ZGPU_COALESCE batching (lazy, under mu)

  Lane *acquire_lane() {
    std::unique_lock<std::mutex> lk(lane_mu);
    while (lanes_free.empty()) {
      if (lanes_all.size() < max_lanes) {
        auto L = std::make_unique<Lane>();
        HIPCHK(hipSetDevice(device));
        HIPCHK(lane_stream_create(&L->stream, device));
        lanes_all.push_back(L.get());
        lanes_free.push_back(L.release());
        break;
      }
      lane_cv.wait(lk);
    }
    Lane *L = lanes_free.back();
    lanes_free.pop_back();
    return L;
  }
  void release_lane(Lane *L) {
    {
      std::lock_guard<std::mutex> lk(lane_mu);
      lanes_free.push_back(L);
    }
    lane_cv.notify_one();
  }

  // Device pool: sizes rounded up to classes (1/8 of a power of two above 1 MiB: <= 12.5 % slack) so
  // that buffers of batches of varying size are reused instead of accumulating; the free blocks are
  // capped (ZGPU_POOL_CAP_MB, default 16 GiB: the largest are returned to HIP beyond it). Without the
  // cap, thousands of concurrent per-chunk calls (the codec plugin's pattern) of varying batch sizes
  // grew the pool until the device had no memory left for a kernel's scratch.
  size_t free_dev_bytes = 0;
  size_t pool_cap = (size_t)16 << 30;
  static size_t size_class(size_t b) {
    b = std::max<size_t>(256, (b + 255) & ~(size_t)255);
    if (b <= (1u << 20)) return b;
    size_t p = (size_t)1 << (63 - __builtin_clzll(b - 1));  // largest power of two < b
    const size_t step = p / 8;
    return (b + step - 1) / step * step;
  }
  void trim_free_locked(size_t keep) {
    while (free_dev_bytes > keep && !free_dev.empty()) {
      auto it = std::prev(free_dev.end());  // the largest free block
      (void)hipFree(it->second);
      free_dev_bytes -= it->first;
      free_dev.erase(it);
    }
  }
  void *dev_alloc(size_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    bytes = size_class(bytes);
    auto it = free_dev.lower_bound(bytes);
    if (it != free_dev.end() && it->first <= bytes + bytes / 4 + (1u << 20)) {
      void *p = it->second;
      live_dev[p] = it->first;
      free_dev_bytes -= it->first;
      free_dev.erase(it);
      return p;
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {  // release the cache and retry once
      (void)hipGetLastError();
      trim_free_locked(0);
      HIPCHK(hipMalloc(&p, bytes));
    }
    live_dev[p] = bytes;
    return p;
  }
  void dev_free(void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    auto it = live_dev.find(p);
    if (it == live_dev.end()) return;
    free_dev.emplace(it->second, p);
    free_dev_bytes += it->second;
    live_dev.erase(it);
    if (free_dev_bytes > pool_cap) trim_free_locked(pool_cap / 2);
  }
  // Pinned host pool: the same size classes, free blocks capped at ZGPU_PINNED_CAP_MB (default 4 GiB;
  // the largest go back to HIP beyond it) -- per-chunk pinned results of varying size otherwise
  // accumulate a free block per distinct size
  size_t free_host_bytes = 0;
  size_t host_cap = (size_t)4 << 30;
  void trim_host_locked(size_t keep) {
    while (free_host_bytes > keep && !free_host.empty()) {
      auto it = std::prev(free_host.end());
      (void)hipHostFree(it->second);
      free_host_bytes -= it->first;
      free_host.erase(it);
    }
  }
  void *host_alloc(size_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    bytes = std::max<size_t>(4096, size_class((bytes + 4095) & ~(size_t)4095));
    auto it = free_host.lower_bound(bytes);
    if (it != free_host.end() && it->first <= bytes + bytes / 4 + (1u << 20)) {
      void *p = it->second;
      live_host[p] = it->first;
      free_host_bytes -= it->first;
      free_host.erase(it);
      return p;
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {  // release the cache and retry once
      (void)hipGetLastError();
      trim_host_locked(0);
      HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    }
    live_host[p] = bytes;
    return p;
  }
  void host_free(void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu);
    auto it = live_host.find(p);
    if (it == live_host.end()) return;
    free_host.emplace(it->second, p);
    free_host_bytes += it->second;
    live_host.erase(it);
    if (free_host_bytes > host_cap) trim_host_locked(host_cap / 2);
  }
  ~zgpu_ctx() {
    (void)hipSetDevice(device);
    for (Lane *L : lanes_all) {
      if (L->stream) (void)hipStreamSynchronize(L->stream);
      if (L->out_hi) (void)hipStreamSynchronize(L->out_hi);
    }
    for (auto &kv : free_dev) (void)hipFree(kv.second);
    for (auto &kv : live_dev) (void)hipFree(kv.first);
    for (auto &kv : free_host) (void)hipHostFree(kv.second);
    for (auto &kv : live_host) (void)hipHostFree(kv.first);
    for (Lane *L : lanes_all) {
      if (L->stream) (void)hipStreamDestroy(L->stream);
      if (L->order_ev) (void)hipEventDestroy(L->order_ev);
      if (L->out_hi) (void)hipStreamDestroy(L->out_hi);
      for (hipStream_t cs : L->copy)
        if (cs) (void)hipStreamDestroy(cs);
      delete L;
    }
    if (peer) (void)hipStreamDestroy(peer);
    delete_coalescer(co);
    (void)hipGetLastError();  // teardown failures must not surface in the caller's next HIP error check
  }
};

// A call's lane for its whole duration (RAII).
struct LaneScope {
  zgpu_ctx *C;
  Lane *L;
  explicit LaneScope(zgpu_ctx *c) : C(c), L(c->acquire_lane()) {}
  ~LaneScope() { C->release_lane(L); }
  LaneScope(const LaneScope &) = delete;
  LaneScope &operator=(const LaneScope &) = delete;
};

// Blocks of a context's pools with one owner: a block is on the owner's list before its pointer is
// handed out, and release() (or the destructor) gives every block back. A plan owns its buffers this
// way for its lifetime; nothing here waits for a stream.
class PoolBlocks {
  zgpu_ctx *C;
  std::vector<void *> dev_, pin_;

 public:
  explicit PoolBlocks(zgpu_ctx *c) : C(c) {}
  ~PoolBlocks() { release(); }
  PoolBlocks(const PoolBlocks &) = delete;
  PoolBlocks &operator=(const PoolBlocks &) = delete;
  template <class T>
  T *dev(size_t count) {
    dev_.push_back(nullptr);
    return (T *)(dev_.back() = C->dev_alloc(count * sizeof(T)));
  }
  template <class T>
  T *pinned(size_t count) {
    pin_.push_back(nullptr);
    return (T *)(pin_.back() = C->host_alloc(count * sizeof(T)));
  }
  // a device block of this owner swapped for one of `bytes` (the old block goes back first)
  void *regrow(void *old, size_t bytes) {
    if (!old) return dev<uint8_t>(bytes);
    auto it = std::find(dev_.begin(), dev_.end(), old);
    if (it == dev_.end()) return dev<uint8_t>(bytes);  // (not one of this owner's: left alone)
    C->dev_free(old);
    *it = nullptr;
    return *it = C->dev_alloc(bytes);
  }
  bool empty() const { return dev_.empty() && pin_.empty(); }
  void release() {
    for (void *p : dev_) C->dev_free(p);
    for (void *p : pin_) C->host_free(p);
    dev_.clear();
    pin_.clear();
  }
};

// A call's temporaries on stream s. One rule for every site: nothing goes back to the pool while work
// touching it may still be queued, so the destructor synchronises s (error ignored: it runs on the
// way out of a failed call too) before it returns the blocks. The pool is shared by all lanes, and a
// block freed early could be handed to a concurrent call on another lane.
class Scratch : PoolBlocks {  // (no regrow, no early release: allocate, and let the scope end)
  hipStream_t s;

 public:
  Scratch(zgpu_ctx *c, hipStream_t stream) : PoolBlocks(c), s(stream) {}
  ~Scratch() {
    if (!empty()) (void)hipStreamSynchronize(s);
  }
  using PoolBlocks::dev;
  using PoolBlocks::pinned;
};
#pragma GCC visibility pop
