// Internals shared by the translation units that implement the C ABI (mh_api.hip, chain_api.hip, photo_api.hip, ...): the context,
// error plumbing, the device / pinned allocation cache and the growable device buffer.  Not installed, not part of
// the boundary.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <set>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mimosa_hip.h"
#include <atomic>

#include "align_device.hpp"
#include "window_device.hpp"
#include "icp_device.hpp"
#include "map_device.hpp"
#include "scan_device.hpp"
#include "shard_device.hpp"
#include "window_request.hpp"

inline thread_local std::string g_mh_err;
constexpr int kMaxPending = 64;
constexpr int kMaxBatch = 64;  // factors per mh_icp_linearize_batch call

struct WindowLaunch
{
  int tpb, k, n_off, first, n, grid;  // one staged K3 launch per iteration: class, kernel path, its first slot and members, its grid
};
// What every chain over several factors keeps of them while it is in flight (a window's poses, an alignment chain's members).
constexpr int kChainMax = 16;
static_assert(kChainMax == mh::kWindowMax && kChainMax == MH_ALIGN_BATCH_MAX, "one member table for the window and the alignment chains");
struct ChainMembers
{
  int queued = 0, n_slots = 0;  // iterations on the stream so far; argument blocks per iteration
  mh_icp * icps[kChainMax];
  int slot[kChainMax];  // member i's argument block within an iteration (-1: a factor that runs no K3)
  int count0[kChainMax];  // its linearize count and its pose when the call began
  double R0[kChainMax][9];
  double gz[3];
  unsigned int seq[64];  // one sequence number per iteration
  std::vector<WindowLaunch> launches;
};
// mh_icp_window_optimise (chain_api.hip): the call in flight on a context (at most one).  Its argument blocks, grid prefixes, state and K3's
// landing slots live in device memory the context owns (d_window), their pinned staging in h_window, the rows the step
// kernel publishes in mapped pinned memory (h_window_rows).
struct WindowCall : ChainMembers
{
  bool active = false;
  int W = 0, iters = 0;
  mh::WindowParams p;
  // optimise: iterations of K3 and a step kernel, the result to outputs.out; marginal / marginal_joint: one K3 launch of icps[0]
  // and the (joint) marginal kernel, the result to outputs.marg / outputs.jmarg
  WindowKind kind = WindowKind::optimise;
  WindowOutputs outputs;
  bool has_joint = false;  // the call carries a joint factor (optimise: the joint step kernel; marginal_joint: absorbed)
  // the features of an optimise call, which choose its step kernel (window_enqueue)
  bool relin = false;  // mh_icp_window_optimise_relin: the step kernel chooses per factor and iteration whether K3 runs
  double relin_rot = 0.0, relin_trans = 0.0;
  bool lin = false;    // mh_icp_window_optimise_lin: the step kernel also carries the call's linear factors
  bool edges = false;  // mh_icp_window_optimise_edges with n_edges > 0: ... and the call's edges, solved over the row profile
  double L1R[9], L1t[3];  // marginal: pose 1 as the caller gave it
  int n_sep = 0, sep[MH_WINDOW_JOINT_POSES];                                   // marginal_joint: its separator
  double LSR[MH_WINDOW_JOINT_POSES][9], LSt[MH_WINDOW_JOINT_POSES][3];         // ... and those poses as the caller gave them
};

// An alignment chain (chain_api.hip): the mh_icp_align call in flight on a factor (mh_icp::align, capacity 1) or the
// mh_icp_align_batch call in flight on a context (mh_ctx::align_batch, capacity MH_ALIGN_BATCH_MAX); at most one of each.  Its
// argument blocks, grid prefixes, the members' AlignStates and K3's landing slots live in the device block `d`, the pinned
// staging of the first part in `h`; whoever owns the record owns both.  Every member's rows arrive in that member's own pinned
// ring.  The block, as a function of the capacity:
// [grid prefixes, 256 B | capacity x AlignState at a 192 B stride | max_iters x n_slots argument blocks | 256 B that load_uniform
//  may read past the last block | one landing slot of 32 flagged words per member for K3's sums and counters (every iteration's
//  words carry its own number, and the step that reads them is on the stream in front of the next K3)]
constexpr size_t kAlignStateAt = 256;
constexpr size_t kAlignStateStride = 192;
constexpr size_t kAlignLlWords = 32;
constexpr size_t align_blocks_at(int capacity) { return (kAlignStateAt + kAlignStateStride * static_cast<size_t>(capacity) + 255) & ~size_t(255); }
constexpr size_t align_stage_bytes(int capacity) { return align_blocks_at(capacity) + sizeof(mh::IcpArgs) * static_cast<size_t>(capacity) * kMaxPending; }
constexpr size_t align_ll_at(int capacity) { return (align_stage_bytes(capacity) + 256 + 255) & ~size_t(255); }
constexpr size_t align_bytes(int capacity) { return align_ll_at(capacity) + kAlignLlWords * sizeof(uint4) * static_cast<size_t>(capacity); }
static_assert(sizeof(mh::AlignState) <= kAlignStateStride && mh::kRowWords <= mh::kLlEig && MH_ALIGN_BATCH_MAX == mh::kAlignBatchMax &&
                2 * MH_ALIGN_BATCH_MAX * sizeof(int) <= kAlignStateAt, "alignment chain layout");
struct AlignChain : ChainMembers
{
  explicit AlignChain(int members_max) : capacity(members_max) {}
  const int capacity;
  int n = 0;  // members of the call in flight (0: none)
  const char * what = "";  // the entry point's name, for its messages
  mh_icp_align_config cfg{};
  mh::AlignParams p[kChainMax];
  mh_icp_align_result * out = nullptr;  // n of them
  void * h = nullptr, * d = nullptr;
};

// A handle that may outlive its context: it is listed on the context from create to destroy.  mh_shutdown waits for the stream
// once, then tells every listed handle (ctx_gone: give the device and pinned memory back while the context is alive) and leaves
// it with ctx == nullptr; from then on every entry point refuses the handle (ctx_alive) and its destroy just deletes it.
struct CtxOwned
{
  mh_ctx * ctx = nullptr;
  virtual void ctx_gone() = 0;

protected:
  ~CtxOwned() = default;
};

struct mh_ctx
{
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = true;  // false: adopted from the caller (mh_init_on_stream)
  std::string err;
  int profiling = 0;  // 0 off; n: HIP events around the kernels of every n-th linearize call of a factor
  hipEvent_t timer[2] = {nullptr, nullptr};
  void * h_batch = nullptr;  // pinned staging of mh_icp_linearize_batch's argument blocks
  void * d_batch = nullptr;  // ... and the device copy the batched kernels read
  void * d_scratch = nullptr;  // stream-ordered scratch of factor creation (source ordering): reused, never freed per call
  size_t d_scratch_cap = 0;
  void * h_window = nullptr;       // mh_icp_window_optimise: pinned staging of the chain's block
  void * d_window = nullptr;       // ... the block itself
  uint4 * h_window_rows = nullptr; // ... the rows of its iterations (mapped pinned), and their device-side address
  uint4 * d_window_rows = nullptr;
  WindowCall window;
  AlignChain align_batch{MH_ALIGN_BATCH_MAX};  // mh_icp_align_batch: its storage is allocated at the first call and freed by mh_shutdown
  hipStream_t copy_stream = nullptr;  // mh_scan_prefetch: uploads beside the compute stream (created on first use: an HSA queue costs ~1 ms)
  std::mutex copy_mu;
  // what mh_shutdown takes back from the sharded handles (shard_api.hip): the sharded factors created on this context, and
  // the communicators whose rounds run on it
  std::vector<mh_shard_icp *> shard_factors;
  std::vector<mh_shard_comm *> shard_comms;
  // ... and the handles that may outlive it (CtxOwned: place databases, pose graphs, keyframe stores)
  std::vector<CtxOwned *> owned;
};

// The stream of the context the calling thread is working for (set by mh_enter at every entry point): what the allocation
// cache orders its hand-overs by.
inline thread_local hipStream_t g_mh_stream = nullptr;
inline hipError_t mh_enter(const mh_ctx * ctx)
{
  g_mh_stream = ctx->stream;
  return hipSetDevice(ctx->device);
}
// While one of these lives, the blocks the calling thread frees go back to the cache as drained (AllocCache::free): a destroy
// function constructs it AFTER it has waited for every stream that touched the handle's buffers, around the `delete` that
// runs their destructors.
inline thread_local bool g_mh_drained = false;
struct DrainedScope
{
  const bool was = g_mh_drained;
  DrainedScope() { g_mh_drained = true; }
  DrainedScope(const DrainedScope &) = delete;
  DrainedScope & operator=(const DrainedScope &) = delete;
  ~DrainedScope() { g_mh_drained = was; }
};

inline int fail(const mh_ctx * ctx, int code, const std::string & msg)
{
  g_mh_err = msg;
  if (ctx) const_cast<mh_ctx *>(ctx)->err = msg;
  return code;
}
// CtxOwned: listed at create, unlisted at destroy (a no-op once the context is gone), and what every other entry point asks first
// (noun: "database", "graph", "store")
inline void ctx_register(CtxOwned * h, mh_ctx * ctx)
{
  h->ctx = ctx;
  ctx->owned.push_back(h);
}
inline void ctx_unregister(CtxOwned * h)
{
  if (!h->ctx) return;
  auto & v = h->ctx->owned;
  v.erase(std::remove(v.begin(), v.end(), h), v.end());
}
inline int ctx_alive(const CtxOwned * h, const char * who, const char * noun)
{
  if (h->ctx) return MH_OK;
  return fail(nullptr, MH_ERR_INVALID_ARG, std::string(who) + ": the " + noun + "'s context was shut down; the handle can only be destroyed");
}
inline int hip_fail(const mh_ctx * ctx, hipError_t e, const char * what)
{
  const int code = (e == hipErrorOutOfMemory) ? MH_ERR_OOM : (e == hipErrorNoDevice ? MH_ERR_NO_DEVICE : MH_ERR_HIP);
  return fail(ctx, code, std::string(what) + ": " + hipGetErrorString(e));
}
// Nothing throws across the C boundary (include/mimosa_hip.h): every extern "C" body runs inside this.
template <typename E>
inline int guarded(const mh_ctx * ctx, const char * what, E && body)
{
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return fail(ctx, MH_ERR_OOM, std::string(what) + ": host allocation failed");
  } catch (const std::exception & e) {
    return fail(ctx, MH_ERR_HIP, std::string(what) + ": " + e.what());
  } catch (...) {
    return fail(ctx, MH_ERR_HIP, std::string(what) + ": unknown exception");
  }
}
#define MH_HIP(ctx, call)                                   \
  do {                                                      \
    const hipError_t e_ = (call);                           \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call);  \
  } while (0)

// Device / pinned-host allocation cache.  A scan creates a factor (a dozen device buffers, a pinned result
// ring, sort temporaries) and destroys it a few hundred milliseconds later; hipMalloc / hipFree / hipHostMalloc
// cost 10-200 us each and hipFree synchronises the device.  Freed blocks of 4 KiB .. 64 MiB are kept per
// (device, rounded size) and handed out again; the cache holds at most kMaxCachedBytes per device.
// Hand-over is STREAM-ORDERED, there is no device-wide drain: a block freed while its last user may still be running
// carries an event recorded on the freeing thread's stream (g_mh_stream: every piece of work on the block was enqueued there
// before the free); whoever takes the block next on the same stream simply queues behind, on another stream waits for the
// event on the device.  (Round 2 drained the whole device per free, which stalled the photometric stream behind the
// geometric one and vice versa.)
// MH_ALLOC_CHECK=1 (environment, diagnostic): the rule above is CHECKED.  Every block that goes back to the cache is
// poisoned on the freeing stream (a fill behind everything that stream enqueued on it, in front of the release event), and
// every cached block that is handed out again is verified on the taker's stream behind the event: a word that is not the
// poison pattern any more was written by work that was NOT ordered in front of the free — a user on another stream the
// freeing thread did not wait for.  Reads of that kind see the pattern and fail the parity suites.  Violations are counted
// in mapped host memory (mh_alloc_check_stats) and reported when the last context of the process is shut down.
namespace mh
{
hipError_t launch_alloc_verify(const void * p, size_t bytes, unsigned long long * violations, hipStream_t stream);  // mh_api.hip
}
constexpr unsigned int kAllocPoison = 0xA5C3A5C3u;

class AllocCache
{
public:
  static bool checking()
  {
    static const bool on = [] {
      const char * e = std::getenv("MH_ALLOC_CHECK");
      return e && *e && *e != '0';
    }();
    return on;
  }
  // [0] blocks verified at hand-out, [1] words found overwritten; mapped pinned (the verify kernel adds to [1])
  static unsigned long long * check_counters()
  {
    static unsigned long long * c = [] {
      void * p = nullptr;
      if (hipHostMalloc(&p, 2 * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) return static_cast<unsigned long long *>(nullptr);
      std::memset(p, 0, 2 * sizeof(unsigned long long));
      return static_cast<unsigned long long *>(p);
    }();
    return c;
  }
  static hipError_t alloc(void ** out, size_t bytes)
  {
    const size_t cls = size_class(bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (cls) {
      Cached c{};
      if (take(dev, cls, true, c)) {
        hand_over(c, dev, cls);
        *out = c.p;
        return hipSuccess;
      }
    }
    static const bool trace = std::getenv("MH_ALLOC_TRACE") != nullptr;  // every trip to the runtime, with its cost, on stderr
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(out, cls ? cls : bytes);
    if (trace)
      std::fprintf(stderr, "AllocCache: hipMalloc(%zu) %.0f us (stream %p)\n", cls ? cls : bytes,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), static_cast<void *>(g_mh_stream));
    if (e != hipSuccess && cls) {
      // out of memory: a cached block that is still in flight on another stream is better than none
      (void)hipGetLastError();
      Cached c{};
      if (take(dev, cls, false, c)) {
        hand_over(c, dev, cls);
        *out = c.p;
        return hipSuccess;
      }
      return e;
    }
    if (e == hipSuccess && cls) {
      std::lock_guard<std::mutex> g(mu());
      live()[*out] = Block{cls, dev};
    }
    return e;
  }
  // drained: the caller has already waited for every stream that ever touched the block (a factor's or a scan's own
  // buffers after a synchronisation of their context's stream — and of the copy stream where one wrote them): it can be
  // handed out at once.  The default is what the enclosing DrainedScope says (none: not drained)
  // (one copy per translation unit, not one per member of every handle's destructor)
  __attribute__((noinline)) static void free(void * p, bool drained = g_mh_drained)
  {
    if (!p) return;
    Block b{0, 0};
    {
      std::lock_guard<std::mutex> g(mu());
      auto it = live().find(p);
      if (it != live().end()) {
        b = it->second;
        live().erase(it);
      }
    }
    if (b.cls) {
      Cached c{p, nullptr, nullptr, false};
      int cur = 0;
      (void)hipGetDevice(&cur);
      const bool same_dev = cur == b.dev;
      if (checking() && same_dev && g_mh_stream) {
        // poison behind the freeing stream's work on the block (for a drained block: behind nothing — it is idle)
        c.poisoned = hipMemsetD32Async(p, static_cast<int>(kAllocPoison), b.cls / 4, g_mh_stream) == hipSuccess;
        if (drained && c.poisoned) drained = false;  // the fill itself is in flight now: hand over behind an event
      }
      if (!drained) {
        if (g_mh_stream && same_dev) {  // (an event of one device cannot be recorded on a stream of another)
          {
            std::lock_guard<std::mutex> g(mu());
            auto & pool = event_pool()[b.dev];
            if (!pool.empty()) {
              c.ev = pool.back();
              pool.pop_back();
            }
          }
          if (!c.ev && hipEventCreateWithFlags(&c.ev, hipEventDisableTiming) != hipSuccess) c.ev = nullptr;
          if (c.ev && hipEventRecord(c.ev, g_mh_stream) == hipSuccess) {
            c.stream = g_mh_stream;
          } else {
            if (c.ev) (void)hipEventDestroy(c.ev);
            c.ev = nullptr;
          }
        }
        if (!c.ev) drain_device(b.dev);  // no stream known for this thread: the old way, on the block's own device
      }
      std::lock_guard<std::mutex> g(mu());
      if (cached_bytes()[b.dev] + b.cls <= kMaxCachedBytes) {
        free_list()[key(b.dev, b.cls)].push_back(c);
        cached_bytes()[b.dev] += b.cls;
        return;
      }
      if (c.ev) event_pool()[b.dev].push_back(c.ev);  // (the block itself goes back to the runtime below: hipFree waits for the device)
    }
    (void)hipFree(p);
  }
  // context bookkeeping (mh_init / mh_shutdown): per device, under the cache mutex
  static void context_created(int dev)
  {
    std::lock_guard<std::mutex> g(mu());
    contexts_of()[dev]++;
  }
  // the device's last context gives its cached blocks back to the runtime (the pinned ones go when no context is left on any
  // device)
  static void context_destroyed(int dev)
  {
    bool last_of_device = false;
    {
      std::lock_guard<std::mutex> g(mu());
      int & n = contexts_of()[dev];
      if (n > 0) --n;
      last_of_device = n == 0;
    }
    if (last_of_device) trim(dev);
  }
  static void trim(int dev)
  {
    std::vector<void *> dead, dead_pinned;
    bool none_left = false;
    {
      std::lock_guard<std::mutex> g(mu());
      for (auto & kv : free_list())
        if (static_cast<int>(kv.first >> 56) == dev) {
          for (const Cached & c : kv.second) {
            dead.push_back(c.p);
            if (c.ev) event_pool()[dev].push_back(c.ev);
          }
          kv.second.clear();
        }
      cached_bytes()[dev] = 0;
      int total = 0;
      for (const auto & kv : contexts_of()) total += kv.second;
      none_left = total == 0;
      if (none_left)
        for (auto & kv : pinned()) {
          dead_pinned.insert(dead_pinned.end(), kv.second.begin(), kv.second.end());
          kv.second.clear();
        }
    }
    for (void * p : dead) (void)hipFree(p);
    for (void * p : dead_pinned) (void)hipHostFree(p);
    if (none_left && checking() && check_counters()) {
      (void)hipDeviceSynchronize();
      std::fprintf(stderr, "MH_ALLOC_CHECK: %llu cached blocks verified at hand-out, %llu overwritten words found\n", check_counters()[0], check_counters()[1]);
      if (check_counters()[1]) std::abort();  // diagnostic mode: a process that broke the rule does not exit quietly
    }
  }

private:
  friend struct PinnedBuf;
  // pinned, mapped blocks, recycled by their EXACT size (PinnedBuf is the only caller)
  static hipError_t alloc_pinned(void ** out, size_t bytes)
  {
    {
      std::lock_guard<std::mutex> g(mu());
      auto & v = pinned()[bytes];
      if (!v.empty()) {
        *out = v.back();
        v.pop_back();
        return hipSuccess;
      }
    }
    static const bool trace = std::getenv("MH_ALLOC_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocMapped);
    if (trace)
      std::fprintf(stderr, "AllocCache: hipHostMalloc(%zu) %.0f us (stream %p)\n", bytes,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), static_cast<void *>(g_mh_stream));
    return e;
  }
  static void free_pinned(void * p, size_t bytes)
  {
    if (!p) return;
    {
      std::lock_guard<std::mutex> g(mu());
      auto & v = pinned()[bytes];
      if (v.size() < 64) {
        v.push_back(p);
        return;
      }
    }
    (void)hipHostFree(p);
  }
  static std::unordered_map<int, int> & contexts_of()
  {
    static std::unordered_map<int, int> m;
    return m;
  }
  struct Block
  {
    size_t cls;
    int dev;
  };
  struct Cached
  {
    void * p;
    hipStream_t stream;  // where the free was ordered; null with ev == null: nobody is using the block
    hipEvent_t ev;
    bool poisoned;       // MH_ALLOC_CHECK: filled with kAllocPoison behind its last use
  };
  static void drain_device(int dev)
  {
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    (void)hipDeviceSynchronize();
    if (cur != dev) (void)hipSetDevice(cur);
  }
  // a cached block of the class, preferring (prefer_idle) one nobody can still be using or whose last use was ordered on
  // THIS stream: taking another stream's block makes this stream wait (on the device) for that stream to get there
  static bool take(int dev, size_t cls, bool prefer_idle, Cached & c)
  {
    std::lock_guard<std::mutex> g(mu());
    auto & v = free_list()[key(dev, cls)];
    if (v.empty()) return false;
    size_t pick = v.size() - 1;
    if (prefer_idle)
      for (size_t i = v.size(); i-- > 0;)
        if (!v[i].ev || v[i].stream == g_mh_stream) {
          pick = i;
          break;
        }
    c = v[pick];
    v[pick] = v.back();
    v.pop_back();
    cached_bytes()[dev] -= cls;
    live()[c.p] = Block{cls, dev};
    return true;
  }
  // order the taker behind the block's release; a wait that cannot be set up (a stale stream after mh_shutdown, an event the
  // runtime rejects) falls back to draining the block's device — never hands the block out unordered
  static void hand_over(Cached & c, int dev, size_t cls)
  {
    if (c.ev) {
      hipError_t e = hipSuccess;
      if (!g_mh_stream)
        e = hipEventSynchronize(c.ev);
      else if (c.stream != g_mh_stream)
        e = hipStreamWaitEvent(g_mh_stream, c.ev, 0);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (hipEventSynchronize(c.ev) != hipSuccess) {
          (void)hipGetLastError();
          drain_device(dev);
        }
      }
      std::lock_guard<std::mutex> g(mu());
      event_pool()[dev].push_back(c.ev);
      c.ev = nullptr;
    }
    if (c.poisoned && checking() && check_counters()) {
      if (g_mh_stream) {
        __atomic_fetch_add(&check_counters()[0], 1ull, __ATOMIC_RELAXED);
        (void)mh::launch_alloc_verify(c.p, cls, check_counters() + 1, g_mh_stream);
      }
      c.poisoned = false;
    }
  }
  // events are per DEVICE: one recorded on another device's stream fails, and every free would fall back to draining the
  // device
  static std::unordered_map<int, std::vector<hipEvent_t>> & event_pool()
  {
    static std::unordered_map<int, std::vector<hipEvent_t>> v;
    return v;
  }
  static constexpr size_t kMaxCachedBytes = size_t(2) << 30;
  static size_t size_class(size_t bytes)
  {
    if (bytes > (size_t(64) << 20)) return 0;  // big (map-sized) blocks are not cached
    size_t c = 4096;
    while (c < bytes) c += c / 2 >= 4096 ? (c / 4) : c;  // 4K, 8K, 16K, 20K, 25K, ... (~25 % steps)
    return c;
  }
  static uint64_t key(int dev, size_t cls) { return (static_cast<uint64_t>(dev) << 56) | cls; }
  static std::mutex & mu()
  {
    static std::mutex m;
    return m;
  }
  static std::unordered_map<uint64_t, std::vector<Cached>> & free_list()
  {
    static std::unordered_map<uint64_t, std::vector<Cached>> m;
    return m;
  }
  static std::unordered_map<void *, Block> & live()
  {
    static std::unordered_map<void *, Block> m;
    return m;
  }
  static std::unordered_map<int, size_t> & cached_bytes()
  {
    static std::unordered_map<int, size_t> m;
    return m;
  }
  static std::unordered_map<size_t, std::vector<void *>> & pinned()
  {
    static std::unordered_map<size_t, std::vector<void *>> m;
    return m;
  }
};

template <typename T>
inline hipError_t dev_alloc(T ** out, size_t bytes)
{
  void * p = nullptr;
  const hipError_t e = AllocCache::alloc(&p, bytes);
  *out = static_cast<T *>(p);
  return e;
}
inline void dev_free(void * p) { AllocCache::free(p); }

// Scoped device temporary: released (back to the cache) on every exit path, including the early returns of MH_HIP.
template <typename T>
struct DevTemp
{
  T * p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp &) = delete;
  DevTemp & operator=(const DevTemp &) = delete;
  ~DevTemp() { dev_free(p); }
  hipError_t alloc(size_t bytes) { return dev_alloc(&p, bytes ? bytes : 16); }
  operator T *() const { return p; }
};

// Growable device buffer.  Owns its block: move-only, and the destructor gives the block back to the cache (as drained inside a
// DrainedScope, behind an event otherwise).
struct DevBuf
{
  void * p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf & operator=(const DevBuf &) = delete;
  DevBuf(DevBuf && o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf & operator=(DevBuf && o) noexcept
  {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf()
  {
    if (p) AllocCache::free(p);
  }
  // exactly `bytes` (rounded by the cache alone), for the blocks of fixed size; what was held before is released
  hipError_t alloc(size_t bytes)
  {
    release();
    const hipError_t e = AllocCache::alloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  template <typename T>
  T * as() const
  {
    return static_cast<T *>(p);
  }
  hipError_t reserve(size_t bytes, hipStream_t stream, bool keep)
  {
    if (bytes <= cap) return hipSuccess;
    size_t ncap = cap ? cap : 4096;
    while (ncap < bytes) ncap += ncap / 2 + 4096;
    void * np = nullptr;
    hipError_t e = AllocCache::alloc(&np, ncap);
    if (e != hipSuccess) return e;
    if (keep && p && cap) {
      e = hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) {
        AllocCache::free(np, false);
        return e;
      }
    }
    if (p) AllocCache::free(p, false);  // (growth is mid-life: work on the old block may be in flight)
    p = np;
    cap = ncap;
    return hipSuccess;
  }
  void release(bool drained = g_mh_drained)
  {
    if (p) AllocCache::free(p, drained);
    p = nullptr;
    cap = 0;
  }
};

// Pinned (mapped) host block from the cache: the pinned counterpart of DevBuf.  It remembers the size it was taken with, which
// is the size the cache files it under again.
struct PinnedBuf
{
  void * p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf & operator=(const PinnedBuf &) = delete;
  PinnedBuf(PinnedBuf && o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  PinnedBuf & operator=(PinnedBuf && o) noexcept
  {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  // At least `bytes`; the contents are NOT kept, and nothing may still be reading the old block.  A block that grows is taken
  // with `capacity` bytes (a fixed size, or a site's own rounding), by default with the power-of-two class from 64 KiB: the
  // cache recycles by exact size, so sizes that repeat are what makes it hit.
  hipError_t reserve(size_t bytes, size_t capacity = 0)
  {
    if (bytes <= cap) return hipSuccess;
    if (!capacity)
      for (capacity = size_t(64) << 10; capacity < bytes;) capacity <<= 1;
    release();
    const hipError_t e = AllocCache::alloc_pinned(&p, capacity);
    if (e == hipSuccess) cap = capacity;
    return e;
  }
  template <typename T>
  T * as() const
  {
    return static_cast<T *>(p);
  }
  void release()
  {
    AllocCache::free_pinned(p, cap);
    p = nullptr;
    cap = 0;
  }
};

// ---- cloud sources: what the entry points that take a point cloud share ("Cloud sources") -----------------------------
// A cloud on the device: n points `stride` floats apart, xyz first.  What every consumer of a cloud reads.
struct DeviceCloud
{
  const float * d = nullptr;
  size_t n = 0, stride = 3;
};
constexpr size_t kCloudMax = 0x3fffffffu;  // points per batch: what the 32-bit indices of the kernels leave room for
inline int check_stride(const mh_ctx * ctx, const char * who, size_t stride) { return stride >= 3 ? MH_OK : fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": stride_floats must be >= 3"); }
inline int check_rt_pair(const mh_ctx * ctx, const char * who, const void * R, const void * t) { return !R == !t ? MH_OK : fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": R and t go together"); }
inline int check_cloud_size(const mh_ctx * ctx, const char * who, size_t n) { return n <= kCloudMax ? MH_OK : fail(ctx, MH_ERR_UNSUPPORTED, std::string(who) + ": batch too large"); }
// A host cloud on its way to the device: packed xyz in a pinned block (a pageable strided source would copy at a few GB/s), uploaded
// behind everything on the context's stream.  A member of its handle's buffers.  The next upload rewrites the pinned block, so
// whoever uploads waits for the stream before it returns (each caller says where).
struct HostStage
{
  PinnedBuf h;
  DevBuf d;
  int upload(const mh_ctx * ctx, const float * xyz, size_t n, size_t stride, DeviceCloud * out)
  {
    const size_t bytes = n * 3 * sizeof(float);
    if (n) {
      MH_HIP(ctx, h.reserve(bytes));
      MH_HIP(ctx, d.reserve(bytes, ctx->stream, false));
      if (stride == 3)
        std::memcpy(h.p, xyz, bytes);
      else
        for (size_t i = 0; i < n; ++i) std::memcpy(h.as<float>() + 3 * i, xyz + i * stride, 3 * sizeof(float));
      MH_HIP(ctx, hipMemcpyAsync(d.p, h.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    *out = DeviceCloud{d.as<const float>(), n, 3};
    return MH_OK;
  }
};

// device-resident scan front end (mh_scan_*): state of one scan
struct mh_scan
{
  mh_ctx * ctx;
  DevBuf d_raw, d_full, d_geo_idx, d_unique, d_body, d_ds, d_kept_idx, d_counters, d_rt;
  DevBuf d_full_raw;  // points_raw_ (lidar/manager.cpp:376-380): points_full_ as it was before deskewing, kept for the photometric path
  bool keep_raw = false, raw_valid = false;
  DevBuf d_sensor;       // other sensors (mh_scan_prepare_input_layout): raw records, organise-by-ring scratch
  DevBuf d_prep, d_vox;  // scratch of launch_prepare_input / launch_preprocess (scan_device.hpp: prepare_layout, voxel_layout)
  PinnedBuf h_c;  // pinned landing buffer: the device counters (a ScanCounters), then the first kUniqueCached distinct timestamps
  static constexpr size_t kUniqueCached = 4096;
  size_t n_unique_cached = 0;        // how many of unique_ns_ sit behind h_c (0 = ask the device)
  mh::ScanCounters c{};
  size_t n_in = 0, n_body = 0;
  bool prepared = false, preprocessed = false;
  // mh_scan_prefetch: the NEXT cloud staged (pinned buffer -> d_raw on a copy stream of its own) while another scan is processed
  hipEvent_t copy_done = nullptr;
  hipEvent_t compute_mark = nullptr;  // recorded on the compute stream at every prefetch: the copy stream queues behind it
  PinnedBuf h_stage;
  size_t n_prefetched = 0;
  bool prefetch_valid = false;
  // mh_scan_deskew: the poses travel through a pinned block of the scan's own, so the call neither touches the caller's
  // (pageable) buffer from the stream nor waits for it
  PinnedBuf h_rt;
  hipEvent_t rt_done = nullptr;
  // mh_scan_deskew_imu: the IMU intervals travel the same way (h_rt -> d_imu); d_pose = [timestamps | double[12] per group], the
  // table the photometric frame and mh_scan_get_deskew_poses read; the float cast goes into d_rt, where K1 reads it
  DevBuf d_imu, d_pose;
  bool imu_deskewed = false;  // the current cloud was deskewed by mh_scan_deskew_imu: d_pose is its table
};
// the two flag words behind a scan's pinned landing block [ScanCounters | kUniqueCached timestamps | flags]: [0] a ring number
// >= 128 (mh_scan_prepare_input_layout), [1] deskew_pose_kernel met a timestamp behind the last IMU interval
inline uint32_t * scan_pinned_flag(const mh_scan * s)
{
  return reinterpret_cast<uint32_t *>(s->h_c.as<char>() + sizeof(mh::ScanCounters) + mh_scan::kUniqueCached * sizeof(uint32_t));
}
// for the calls that have just waited for the device: what the pose kernel could not report by throwing (lidar/manager.cpp:469-476
// runs off the end of the IMU buffer there)
inline int scan_imu_error(const mh_scan * s, const mh_ctx * ctx, const char * who)
{
  if (s && s->imu_deskewed && s->h_c.p && scan_pinned_flag(s)[1])
    return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": deskewPoints: IMU samples end before the last point of the cloud");
  return MH_OK;
}

// The stage `which` of a scan — 0 points_full_, 1 Be_cloud_, 2 the downsampled cloud — as mh_point32 records; false: it has not run
inline bool scan_stage(const mh_scan * s, int which, DeviceCloud * c)
{
  if (which < 0 || which > 2 || !s->prepared || (which != 0 && !s->preprocessed)) return false;
  const void * d = which == 0 ? s->d_full.p : (which == 1 ? s->d_body.p : s->d_ds.p);
  *c = DeviceCloud{static_cast<const float *>(d), which == 0 ? s->c.n_full : (which == 1 ? s->n_body : s->c.n_downsampled), sizeof(mh_point32) / sizeof(float)};
  return true;
}
// The one way from (scan, which in 0..1) to the cloud a consumer reads.  The checks, in this order: which, the stage has run,
// residence, a buffer behind a count, the size.  Residence: the same device will do for a consumer that reads the scan's buffers
// after the scan's calls have returned; one that is ordered behind them by the stream alone asks for its own context.
enum class Residence { same_device, same_context };
inline int scan_cloud(const mh_ctx * ctx, const char * who, const mh_scan * scan, int which, Residence residence, DeviceCloud * out)
{
  const auto refuse = [&](const char * why) { return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + why); };  // (no string unless it fails)
  if (which < 0 || which > 1) return refuse(": which must be 0 (points_full_) or 1 (Be_cloud_)");
  if (!scan_stage(scan, which, out)) return refuse(": that stage has not run");
  if (residence == Residence::same_context && scan->ctx != ctx) return refuse(": scan belongs to another context");
  if (scan->ctx->device != ctx->device) return refuse(": scan lives on another device");
  if (out->n && !out->d) return refuse(": that stage has not run");
  return check_cloud_size(ctx, who, out->n);
}

// IncrementalVoxelMapPCL counterpart: the device-resident voxel map (map_device.hpp / map_kernels.hip).  The device
// arrays ARE the map; the host keeps counters only (refreshed from the mapped state after every mutation).
struct mh_map
{
  mh_ctx * ctx = nullptr;
  std::atomic<int> refs{1};
  mh_map_config cfg{};
  double inv_leaf = 0, min_sq = 0;
  DevBuf d_table, d_cells, d_buckets, d_qbuckets, d_vox, d_lru;
  size_t table_cap = 0, vox_cap = 0, block_cap = 0;  // capacities in entries (table slots, voxels, blocks)
  DevBuf d_state;                                    // device counters the kernels maintain (a MapState)
  mh::MapState * h_state = nullptr;                  // pinned host copy
  uint32_t n_voxels = 0, n_blocks = 0;
  uint64_t n_points = 0, lru_counter = 0;
  // insert scratch (grown on demand, reused)
  DevBuf s_pts, s_group, s_seg_vid, s_seg_added, s_blk_new, s_flags, s_pos, s_temp, s_rt, s_shard;
  DevBuf s_preview;  // mh_map_preview_insert*: [too close | voxel full] per segment (n words each), then n outcome bytes
  DevBuf s_carve_img, s_carve_vox;  // mh_map_carve*: the observation image (+ its counter); removed / tested / emptied per voxel
  HostStage in;    // a host batch on its way in; in.d is also where the other calls keep a cloud of their own (shard copy, get_cloud)
  int64_t inserts = 0, upload_bytes = 0, purges = 0;
  int n_off = 0;
  int8_t off[27][3];
  // contexts (= HIP streams) that hold factors on this map: a mutation waits for THEIR streams, not for the whole device
  std::mutex readers_mu;
  std::vector<std::pair<mh_ctx *, int>> readers;
  bool poisoned = false;  // a mutation failed half way (LRU purge, carve): the device arrays and the counters disagree; every later call fails
};

// mh_keyframes_*: the clouds of the keyframes, each in its own frame, packed float4 (x, y, z, 1) in one device arena of fixed size
// (keyframes_api.hip).  An entry holds no pose.  mh_map_rebuild_from_keyframes (map_api.hip) reads it.
struct mh_keyframes final : CtxOwned
{
  mh_keyframes_config cfg{};
  std::vector<uint64_t> offsets{0};  // d_offsets on the host: size() + 1 entries
  std::vector<int64_t> tags;
  // what goes back when the context does
  struct Memory
  {
    DevBuf d_arena;    // float4: capacity_points entries
    DevBuf d_offsets;  // unsigned long long: capacity_keyframes + 1, entry i is points [d_offsets[i], d_offsets[i + 1]) of the arena
    HostStage in;      // a host batch on its way in; in.h is also the landing block of a read-back
  } mem;
  float4 * arena() const { return mem.d_arena.as<float4>(); }
  void ctx_gone() override
  {
    mem = Memory{};
    tags.clear();
    offsets.assign(1, 0);
  }
};

inline void map_add_reader(mh_map * m, mh_ctx * c)
{
  std::lock_guard<std::mutex> g(m->readers_mu);
  for (auto & r : m->readers)
    if (r.first == c) {
      ++r.second;
      return;
    }
  m->readers.emplace_back(c, 1);
}
inline void map_remove_reader(mh_map * m, mh_ctx * c)
{
  std::lock_guard<std::mutex> g(m->readers_mu);
  for (auto & r : m->readers)
    if (r.first == c && r.second > 0) --r.second;
}
// Before a mutation: wait for the streams of the OTHER contexts that hold factors on this map (their kernels may be reading
// it); work on the map's own stream is ordered by the stream.  (Round 2 drained the whole device here.)
inline hipError_t map_wait_readers(mh_map * m)
{
  std::vector<hipStream_t> streams;
  {
    std::lock_guard<std::mutex> g(m->readers_mu);
    for (const auto & r : m->readers)
      if (r.second > 0 && r.first != m->ctx) streams.push_back(r.first->stream);
  }
  for (hipStream_t st : streams) {
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

inline mh::MapView map_view(const mh_map * m)
{
  mh::MapView v;
  v.table = static_cast<const int4 *>(m->d_table.p);
  v.cells = static_cast<const uint32_t *>(m->d_cells.p);
  v.buckets = static_cast<const float4 *>(m->d_buckets.p);
  v.qbuckets = static_cast<const uint4 *>(m->d_qbuckets.p);
  v.inv_leaf = m->inv_leaf;
  v.mask = static_cast<uint32_t>(m->table_cap - 1);
  v.n_off = m->n_off;
  v.mode_idx = m->n_off == 1 ? 0 : (m->n_off == 7 ? 1 : (m->n_off == 19 ? 2 : 3));
  return v;
}

// ---- ICP factor handle (mh_api.hip; shared with shard_api.hip and chain_api.hip) ----------------------------------
// Which chain holds a factor: while one does, the factor's whole ring is the chain's (n_pending == kMaxPending), so every entry
// point that needs the factor free refuses it through n_pending alone, as it refuses one with 64 calls in flight.  The entry
// points that must tell the holders apart (mh_icp_wait, mh_icp_reset, mh_icp_destroy) switch on this.
enum class Held { none, align, align_batch, window, score };

struct PendingCall
{
  mh_icp_result * out;
  double R[9];     // delta rotation (for reg_4_dof's local_z)
  double gz[3];    // global_z = -g_unit
  int parity;
  int linearize_count;
  unsigned int seq;  // the call's sequence number: tags every flagged word its kernels publish (0: nothing was launched)
  bool components;   // K4 ran for this call: loc_*_comp / status_hist are meaningful
  bool seq_has_basis = false;  // ... and published the eigenbases it projected on among the call's flagged words
  int loc_blocks = 0;          // plain factors: K4's workgroups of this call = rows of flagged words the host folds
  bool launched_k4 = false;    // plain factors: the call's sums come from K4's workgroup 0 (else from K3's last block)
  hipEvent_t ev[3];
};

struct mh_icp
{
  mh_ctx * ctx;
  mh_map * map;
  size_t n;
  mh_reg_config cfg;
  bool binary;
  DevBuf d_src, d_qda, d_mean, d_normal, d_status, d_partials, d_ticket, d_dbg, d_perm;
  // plain factors: what K4 reads of a call is the record K3 wrote for it (icp_device.hpp: IcpArgs::rec) and K3's partial rows;
  // K4 follows its K3 on the context's stream, so one of each serves every call of the factor
  DevBuf d_rec;
  bool ordered = false;  // d_src / per-point state are in Morton order, d_perm maps back
  PinnedBuf h_ll;             // pinned, mapped ring of flagged-word slots (icp_device.hpp, uint4): what a plain call's kernels publish
  uint4 * d_h_ll = nullptr;   // its device-side address
  size_t ll_words = 0;        // 16-byte words per slot
  PendingCall pending[kMaxPending];
  int n_pending = 0;
  int parity = 0;
  bool cold = true;
  bool components = true;  // mh_icp_set_components: run K4 (component localizabilities + status histogram) in every linearize
  int linearize_count = 0;
  hipEvent_t events[kMaxPending][3];
  bool events_ready = false;
  unsigned int seq_counter = 0;
  // map-sharded use (mh_icp_shard_*): points migrate between ranks with their association state
  bool no_order = false;  // keep the caller's point order (no Morton re-ordering)
  size_t cap_n = 0;       // per-point arrays are sized for this many points (>= n): room for arrivals of the sharded path
  DevBuf d_origin, x_src, x_qda, x_mean, x_normal, x_status, x_origin;  // origin ids; the second set of arrays pack compacts into
  DevBuf s_keys_a, s_keys_b, s_idx_a, s_idx_b, s_counts, s_temp, d_sums;
  uint32_t * h_counts = nullptr;  // pinned
  bool origin_ready = false, plan_open = false;
  uint32_t n_movers = 0;
  Held held = Held::none;  // set and cleared with n_pending: hold(), let_go()
  // mh_icp_align (chain_api.hip): the factor's own alignment chain, capacity 1.  Its device block comes from the allocation
  // cache (d_align; align.d points into it), and so does its pinned staging (h_align; align.h), at the first call.
  DevBuf d_align;
  PinnedBuf h_align;
  AlignChain align{1};
  // which cloud this is: a fresh number for every created factor, the source's for a clone (mh_icp_relocalise_batch asks
  // whether its work factors are clones of the factor it scores)
  uint64_t cloud_id = 0;
  // mh_icp_score_poses (reloc_api.hip): the call's device block [poses | strided cloud | per-workgroup partials | scores]
  // (d_reloc), its mapped pinned block [winners | poses | scores] (h_reloc), and the call in flight.  Like an alignment it
  // holds the factor (Held::score) until mh_icp_wait collects it; it touches nothing else of the factor.
  DevBuf d_reloc;
  PinnedBuf h_reloc;
  struct ScoreCall
  {
    size_t n_poses = 0;
    mh_pose_score * scores = nullptr;
    int32_t * best = nullptr;
  } score;
};

// A call takes hold of a factor, and lets go of it — of all its factors — when it is over: collected, or abandoned behind a
// drained stream.
inline void hold(mh_icp * icp, Held by)
{
  icp->held = by;
  icp->n_pending = kMaxPending;  // the chain holds the whole ring
}
inline void let_go(mh_icp * icp)
{
  icp->held = Held::none;
  icp->n_pending = 0;
}
inline void let_go(mh_icp * const * icps, int n)
{
  for (int i = 0; i < n; ++i) let_go(icps[i]);
}

// The factors of a window that share a kernel instantiation — launch class, k == 5 or the generic k <= 8 path, neighbour mode,
// unary / binary: one batched K3 (+ one K4) launch (mh_icp_linearize_batch, mh_shard_icp_linearize_batch).
struct LaunchGroup
{
  int tpb, k, n_off;
  bool binary;
  std::vector<size_t> members;        // indices into the call's factor list
  int first = 0, grid = 0, grid4 = 0;  // plain path: the group's first staging slot, its K3 and K4 grids
};

// mh_api.hip internals used by shard_api.hip and chain_api.hip
namespace mhi
{
void pose_delta(const double * Rs, const double * ts, const double * Rt, const double * tt, double * R, double * t);
void finish(const mh_icp * icp, const mh::DeviceResult & d, const PendingCall & pc, mh_icp_result * out);
int icp_create(mh_ctx * ctx, mh_map * map, const mh_point32 * source, const mh_point32 * d_source, size_t n, size_t capacity,
               const mh_reg_config * cfg, int is_binary, mh_icp ** out, bool no_order);
// argument blocks of one linearize call in pending slot n_pending (claimed); no launch
int prepare(mh_icp * icp, const double R_src[9], const double t_src[3], const double * R_tgt, const double * t_tgt, const double g_unit[3],
            mh_icp_result * out, mh::IcpArgs & a, mh::LocArgs & l);
// shard_api.hip: called by mh_shutdown(ctx) so that the sharded handles listed on ctx let go of it
void shard_ctx_gone(mh_ctx * ctx);
// a call's DeviceResult from its flagged words in pending slot `slot` (spin_ns > 0: wait up to that long for words that have
// not arrived); false = something is still missing
bool collect_call(const mh_icp * icp, int slot, const PendingCall & pc, long spin_ns, mh::DeviceResult & d);
// sequence numbers of calls: process-wide, never 0
unsigned int next_call_seq();
// the K3 argument block of a components-off linearize of a unary factor at (R, t), for a chain that launches K3 itself: rec =
// nullptr, rec_n = 0, tail = 1; ll and seq are the chain's to set.  The handle's books (cold, linearize_count, n_pending) are
// on return what they were.
int chain_k3_block(mh_icp * icp, const double R[9], const double t[3], const double g_unit[3], mh::IcpArgs & a);
// chain_api.hip: the launch groups of a window (also mh_icp_linearize_batch's), and mh_icp_wait on a factor whose alignment
// is in flight
std::vector<LaunchGroup> window_launch_groups(mh_icp * const * icps, size_t n_factors);
int align_wait(mh_icp * icp);
// reloc_api.hip: mh_icp_wait on a factor whose mh_icp_score_poses_async is in flight
int score_wait(mh_icp * icp);
// chain_api.hip: what mh_icp_align refuses of a config, worded with the caller's prefixes ("<prefix>max_iters must be ...",
// "<prefix>eps, damping, ... must be >= 0"); mh_icp_align_batch without the guard, for mh_icp_relocalise_batch
int align_check_config(const mh_ctx * ctx, const mh_icp_align_config & cfg, const char * iters_prefix, const char * ranges_prefix);
int align_batch(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3], const mh_icp_align_config * cfg,
                mh_icp_align_result * out);
}  // namespace mhi
