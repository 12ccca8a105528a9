// hostutil.hpp — host-side helpers shared by the C-ABI translation units (status codes,
// device allocation, staging buffer, timing events).
#pragma once
#include "../../include/mcdeskew.h"
#include "internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using mcimpl::fail;
#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(e_ == hipErrorOutOfMemory ? MC_ERR_NOMEM : MC_ERR_HIP, "%s failed: %s", \
                  #expr, hipGetErrorString(e_));                                            \
  } while (0)

#define CHECK_ARG(cond, ...) \
  do {                       \
    if (!(cond)) return fail(MC_ERR_INVALID, __VA_ARGS__); \
  } while (0)

// ------------------------------------------------------------------------------------------------
// growing a buffer of the context (devbuf.hpp)
// ------------------------------------------------------------------------------------------------
// At least n elements in buf, the contents not kept.  The one rule for giving a block back: work
// queued on the main stream may still use it, so that stream drains first — on the reallocation path
// only.  (A block the row stream may use needs sync_all before this: rel_table.)
template <typename Buf>
static inline int ctx_reserve(mc_ctx* c, Buf& buf, size_t n, bool* grew = nullptr) {
  if (buf && n > buf.capacity()) (void)hipStreamSynchronize(c->stream);
  return buf.reserve(n, grew);
}

// At least n elements in buf, the first `keep` kept (devbuf.hpp devbuf_grow_keep: geometric growth): a device copy
// on the main stream, which then drains, so the old block is idle when it goes back.  On failure buf is unchanged.
template <typename Buf>
static inline int ctx_reserve_keep(mc_ctx* c, Buf& buf, size_t keep, size_t n, bool* grew = nullptr) {
  if (buf && n > buf.capacity() && keep == 0) (void)hipStreamSynchronize(c->stream);   // ctx_reserve's rule
  return mcimpl::devbuf_grow_keep(buf, keep, n, [c](void* dst, const void* src, size_t bytes) -> int {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MC_OK;
  }, grew);
}

static inline int ctx_stage(mc_ctx* c, size_t bytes, void** out) {
  if (int r = ctx_reserve(c, c->d_stage, bytes)) return r;
  *out = c->d_stage;
  return MC_OK;
}

// pinned, device-mapped host scratch of at least `bytes` (the zero-copy path of the single calls)
static inline int ctx_pin(mc_ctx* c, size_t bytes, void** out) {
  if (int r = ctx_reserve(c, c->h_pin, bytes)) return r;
  *out = c->h_pin;
  return MC_OK;
}

// Scratch of one host float64 row call: sections of 8-byte words back to back.  Below kZeroCopyRows
// rows it is pinned, device-mapped host memory (the kernel reads and writes host memory: no DMA round
// trips for the reference's per-frame calls), from there on the device staging buffer with DMA on
// the main stream.  The host source of a put() must stay alive until fetch(), the call's one sync.
constexpr int64_t kZeroCopyRows = 1 << 15;
constexpr int kRowBlock = 256;   // threads per workgroup of the row kernels (= mc::kBlock)
struct RowScratch {
  hipStream_t s = nullptr;
  void* base = nullptr;
  bool zero_copy = false;
  int open(mc_ctx* c, int64_t n_rows, size_t words) {
    s = c->stream;
    zero_copy = n_rows < kZeroCopyRows;
    return zero_copy ? ctx_pin(c, words * 8, &base) : ctx_stage(c, words * 8, &base);
  }
  template <typename T = char>
  T* at(size_t word) const { return reinterpret_cast<T*>(static_cast<char*>(base) + 8 * word); }
  int put(size_t word, const void* host, size_t n_words) {
    if (zero_copy) std::memcpy(at(word), host, 8 * n_words);
    else HIPCHK(hipMemcpyAsync(at(word), host, 8 * n_words, hipMemcpyHostToDevice, s));
    return MC_OK;
  }
  int fetch(void* host, size_t word, size_t n_words) {
    if (!zero_copy) HIPCHK(hipMemcpyAsync(host, at(word), 8 * n_words, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (zero_copy) std::memcpy(host, at(word), 8 * n_words);
    return MC_OK;
  }
  int grid(int64_t n) const {   // workgroups of a grid-stride row kernel over n rows (fewer over PCIe)
    return (int)std::min<int64_t>((n + kRowBlock - 1) / kRowBlock, zero_copy ? 1024 : 65536);
  }
};

// doff[f] = rows before frame f (F + 1 entries); also(f) != MC_OK fails frame f after its size check
static inline int frame_offsets(const int64_t* counts, int32_t F, std::vector<int64_t>* doff,
                                const std::function<int(int32_t)>& also = nullptr) {
  doff->assign((size_t)F + 1, 0);
  for (int32_t f = 0; f < F; ++f) {
    CHECK_ARG(counts[f] >= 0, "negative frame size at frame %d", f);
    if (also) if (int r = also(f)) return r;
    (*doff)[f + 1] = (*doff)[f] + counts[f];
  }
  return MC_OK;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
  }
};

// event timing around the hot kernels
static inline hipEvent_t ev_take(mc_ctx* c) {
  if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  // timing-only events: no system-scope fence (no L2 writeback/invalidate between the kernels)
  if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return e;
}
// the pairs of v back into the pool
static inline void ev_recycle(mc_ctx* c, EventPairs& v) {
  for (auto& p : v) { c->ev_pool.push_back(p.first); c->ev_pool.push_back(p.second); }
  v.clear();
}
struct TimedRegion {
  mc_ctx* c; EventPairs* v; hipStream_t s; hipEvent_t e0 = nullptr;
  TimedRegion(mc_ctx* c_, EventPairs* v_, hipStream_t s_) : c(c_), v(v_), s(s_) {
    if (c->timing) { e0 = ev_take(c); if (e0) (void)hipEventRecord(e0, s); }
  }
  ~TimedRegion() {
    if (c->timing && e0) {
      hipEvent_t e1 = ev_take(c);
      if (e1) { (void)hipEventRecord(e1, s); v->emplace_back(e0, e1); }
      else c->ev_pool.push_back(e0);
    }
  }
};

// A pair of timing events for one kernel launched with hipExtLaunchKernel: the runtime stamps
// them from the dispatch itself, so timing adds no marker packets between the step's kernels.
struct LaunchEvents {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit LaunchEvents(mc_ctx* c) : LaunchEvents(c, c->timing) {}
  LaunchEvents(mc_ctx* c, bool on) {
    if (!on) return;
    e0 = ev_take(c);
    e1 = e0 ? ev_take(c) : nullptr;
    if (e0 && !e1) { c->ev_pool.push_back(e0); e0 = nullptr; }
  }
  void keep(EventPairs* v) {
    if (e0) v->emplace_back(e0, e1);
    e0 = e1 = nullptr;
  }
};

// both streams idle (before reallocating anything queued work may still read or write)
static inline int sync_all(mc_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->row_d2h));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

static inline int sum_events(mc_ctx* c, EventPairs& v, double* ms, int64_t* n) {
  double tot = 0.0;
  for (auto& p : v) {
    float m = 0.f;
    HIPCHK(hipEventElapsedTime(&m, p.first, p.second));
    tot += m;
  }
  if (ms) *ms = tot;
  if (n) *n = (int64_t)v.size();
  ev_recycle(c, v);
  return MC_OK;
}

// a mc_timing_read_* of one list: total ms and launches since the last read
static inline int read_timing(mc_ctx* c, EventPairs& v, double* ms, int64_t* n) {
  DeviceGuard g(c->device);
  if (int r = sync_all(c)) return r;
  return sum_events(c, v, ms, n);
}

// a mc_timing_read_* of `count` lists, one per phase (ev null: the feature has no state yet): ms_phase[k]
// = the ms of ev[k] since the last read, zero without a state; *launches = their regions together
static inline int read_timing_phases(mc_ctx* c, EventPairs* ev, int count, double* ms_phase, int64_t* launches) {
  DeviceGuard g(c->device);
  if (int r = sync_all(c)) return r;
  int64_t total = 0;
  for (int k = 0; k < count; ++k) if (ms_phase) ms_phase[k] = 0.0;
  for (int k = 0; ev && k < count; ++k) {
    int64_t n = 0;
    if (int r = sum_events(c, ev[k], ms_phase ? ms_phase + k : nullptr, &n)) return r;
    total += n;
  }
  if (launches) *launches = total;
  return MC_OK;
}

// ------------------------------------------------------------------------------------------------
// a feature's state in its slot of the context (internal.hpp CtxExt)
// ------------------------------------------------------------------------------------------------
// the unit's state S (nullptr: none yet and !create)
template <typename S>
static inline S* ctx_ext(mc_ctx* c, mcimpl::CtxSlot slot, bool create) {
  auto& p = c->ext[slot];
  if (!p && create) p.reset(new S());
  return static_cast<S*>(p.get());
}
// in a state's destructor: its timing pairs nobody read (the context's pool is not its to fill then)
static inline void ev_destroy(EventPairs& v) {
  for (auto& p : v) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  v.clear();
}
