// devbuf.hpp — the one owner of device memory (and of the two pinned host blocks): a move-only
// buffer that frees its block when it dies, so a handle's destructor is its member list.
//
// It never synchronises: what must be idle before a block is given back is the caller's rule
// (hostutil.hpp ctx_reserve).  Every device block it holds is counted in g_live_bytes / g_live_blocks
// (mc_device_memory_live); pinned host blocks and what mc_device_alloc hands to the caller are not.
//
// With MC_DEVBUF_HOST_TEST the two raw calls become malloc / free, failing above g_test_fail_above
// bytes, and no HIP header is read: the type then runs under the sanitizers on a machine with no GPU
// (tests/host/devbuf_host.cpp).
#pragma once
#ifdef MC_DEVBUF_HOST_TEST
#include <cstdlib>
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
#else
#include <hip/hip_runtime_api.h>
#endif
#include <stdint.h>
#include <atomic>
#include <cstddef>
#include <utility>

#include "../../include/mcdeskew.h"

namespace mcimpl {
int fail(int code, const char* fmt, ...);

inline std::atomic<int64_t> g_live_bytes{0}, g_live_blocks{0};

// where a block lives: device memory, or pinned host memory with these hipHostMalloc flags
constexpr int kDeviceMem = -1;

#ifdef MC_DEVBUF_HOST_TEST
inline size_t g_test_fail_above = SIZE_MAX;
inline hipError_t raw_alloc(void** p, size_t bytes, int) {
  if (bytes > g_test_fail_above) return hipErrorOutOfMemory;
  *p = std::malloc(bytes);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline void raw_free(void* p, int) { std::free(p); }
inline const char* raw_error(hipError_t) { return "injected failure"; }
#else
inline hipError_t raw_alloc(void** p, size_t bytes, int where) {
  return where == kDeviceMem ? hipMalloc(p, bytes) : hipHostMalloc(p, bytes, (unsigned)where);
}
inline void raw_free(void* p, int where) {
  if (where == kDeviceMem) (void)hipFree(p);
  else (void)hipHostFree(p);
}
inline const char* raw_error(hipError_t e) { return hipGetErrorString(e); }
#endif

template <typename T, int Where = kDeviceMem>
struct DevBuf {
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  void reset() {
    if (p_) {
      raw_free(p_, Where);
      account(-1);
    }
    p_ = nullptr;
    cap_ = 0;
  }
  // a fresh block of n elements (n == 0: one element); on failure the buffer is empty
  int alloc(size_t n) {
    reset();
    if (n == 0) n = 1;
    void* p = nullptr;
    const hipError_t e = raw_alloc(&p, n * sizeof(T), Where);
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? MC_ERR_NOMEM : MC_ERR_HIP, "allocating %zu bytes failed: %s",
                  n * sizeof(T), raw_error(e));
    p_ = static_cast<T*>(p);
    cap_ = n;
    account(1);
    return MC_OK;
  }
  // grow-only: at least n elements, the contents not kept; *grew: whether the block changed
  int reserve(size_t n, bool* grew = nullptr) {
    if (grew) *grew = false;
    if (n <= cap_) return MC_OK;
    const int r = alloc(n);
    if (grew) *grew = r == MC_OK;
    return r;
  }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  template <typename U>
  U* as() const { return reinterpret_cast<U*>(p_); }   // a byte buffer's records
  size_t capacity() const { return cap_; }              // elements

 private:
  void account(int sign) {
    if (Where != kDeviceMem) return;
    g_live_bytes += sign * (int64_t)(cap_ * sizeof(T));
    g_live_blocks += sign;
  }
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Grow-only with the contents kept: at least n elements in buf, the first `keep` of them what they were.  A new
// block (twice the old capacity when that is more than n, so a stream of small steps copies a record O(1) times;
// exactly n when the larger block cannot be had), copy(dst, src, bytes) — which returns MC_OK only once the bytes
// are there and nothing uses the old block any more — then a move-assign.  On any failure buf is what it was.
template <typename T, int Where, typename Copy>
int devbuf_grow_keep(DevBuf<T, Where>& buf, size_t keep, size_t n, Copy&& copy, bool* grew = nullptr) {
  if (grew) *grew = false;
  if (n <= buf.capacity()) return MC_OK;
  if (keep > buf.capacity()) return fail(MC_ERR_STATE, "keeping %zu elements of a block of %zu", keep, buf.capacity());
  DevBuf<T, Where> next;
  const size_t twice = 2 * buf.capacity();
  if (twice <= n || next.alloc(twice) != MC_OK)
    if (int r = next.alloc(n)) return r;
  if (keep > 0)
    if (int r = copy(static_cast<void*>(next.get()), static_cast<const void*>(buf.get()), keep * sizeof(T))) return r;
  buf = std::move(next);
  if (grew) *grew = true;
  return MC_OK;
}

// pinned host memory: the same body over hipHostMalloc / hipHostFree
template <typename T, unsigned Flags>
using PinBuf = DevBuf<T, (int)Flags>;
}  // namespace mcimpl
