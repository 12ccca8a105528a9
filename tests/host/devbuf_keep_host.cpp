// devbuf_keep_host.cpp — the content-keeping growth of csrc/devbuf.hpp (devbuf_grow_keep, what hostutil.hpp's
// ctx_reserve_keep runs with a device copy) on the host: MC_DEVBUF_HOST_TEST puts malloc / free behind the seam, and
// an allocation above g_test_fail_above bytes fails.  A stand-alone program, built under ASan + UBSan + leak
// detection by tests/test_voxel_insert_cpu.py.  Prints "bad <n>"; exit status 1 when n > 0.
#include "devbuf.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace mcimpl {
int fail(int code, const char*, ...) { return code; }
}  // namespace mcimpl
using mcimpl::DevBuf;
using mcimpl::devbuf_grow_keep;
using mcimpl::g_live_blocks;
using mcimpl::g_live_bytes;
using mcimpl::g_test_fail_above;

static int bad = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) { ++bad; std::printf("line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static bool live(int64_t bytes, int64_t blocks) { return g_live_bytes == bytes && g_live_blocks == blocks; }

static int copies = 0;
static int copy_ok(void* dst, const void* src, size_t bytes) {
  ++copies;
  std::memcpy(dst, src, bytes);
  return MC_OK;
}
static int copy_fails(void*, const void*, size_t) { return MC_ERR_HIP; }

// the first n elements are 0, 1, 2, ...
static bool counts_up(const DevBuf<int64_t>& b, size_t n) {
  for (size_t i = 0; i < n; ++i) if (b.get()[i] != (int64_t)i) return false;
  return true;
}

int main() {
  {  // an empty buffer: a block of exactly n, nothing to copy
    DevBuf<int64_t> b;
    bool grew = false;
    EXPECT(devbuf_grow_keep(b, 0, 5, copy_ok, &grew) == MC_OK && grew && b.capacity() == 5 && copies == 0 && live(40, 1));
    for (int i = 0; i < 5; ++i) b.get()[i] = i;
    // within the capacity: the same block
    int64_t* p = b;
    EXPECT(devbuf_grow_keep(b, 5, 5, copy_ok, &grew) == MC_OK && !grew && b.get() == p && copies == 0);
    EXPECT(devbuf_grow_keep(b, 5, 3, copy_ok, &grew) == MC_OK && !grew && b.get() == p);
    // one more: geometric, twice the old block, the contents kept and the old block given back
    EXPECT(devbuf_grow_keep(b, 5, 6, copy_ok, &grew) == MC_OK && grew && b.capacity() == 10 && copies == 1 && live(80, 1));
    EXPECT(counts_up(b, 5));
    for (int i = 5; i < 10; ++i) b.get()[i] = i;   // every element of the new block is the caller's (ASan checks)
    // far more than twice: exactly n
    EXPECT(devbuf_grow_keep(b, 10, 100, copy_ok, &grew) == MC_OK && grew && b.capacity() == 100 && copies == 2 && live(800, 1));
    EXPECT(counts_up(b, 10));
    // keeping only a prefix
    EXPECT(devbuf_grow_keep(b, 4, 150, copy_ok) == MC_OK && b.capacity() == 200 && copies == 3 && counts_up(b, 4));
    // keep = 0 of a full buffer: a new block, no copy
    EXPECT(devbuf_grow_keep(b, 0, 500, copy_ok) == MC_OK && b.capacity() == 500 && copies == 3 && live(4000, 1));
  }
  EXPECT(live(0, 0));
  {  // a stream of steps of one element copies each element O(1) times: log2 blocks
    DevBuf<int64_t> b;
    copies = 0;
    for (size_t n = 1; n <= 1000; ++n) {
      EXPECT(devbuf_grow_keep(b, n - 1, n, copy_ok) == MC_OK);
      b.get()[n - 1] = (int64_t)(n - 1);
    }
    EXPECT(copies == 10 && b.capacity() == 1024 && counts_up(b, 1000) && live(8192, 1));
  }
  EXPECT(live(0, 0));
  {  // failures leave the buffer as it was
    DevBuf<int64_t> b;
    EXPECT(b.alloc(8) == MC_OK);
    for (int i = 0; i < 8; ++i) b.get()[i] = i;
    int64_t* p = b;
    bool grew = true;
    g_test_fail_above = 100;   // twice (128 bytes) cannot be had, n = 9 (72 bytes) can
    EXPECT(devbuf_grow_keep(b, 8, 9, copy_ok, &grew) == MC_OK && grew && b.capacity() == 9 && counts_up(b, 8) && live(72, 1));
    p = b;
    EXPECT(devbuf_grow_keep(b, 8, 20, copy_ok, &grew) == MC_ERR_NOMEM && !grew && b.get() == p && b.capacity() == 9 && counts_up(b, 8) &&
           live(72, 1));
    g_test_fail_above = SIZE_MAX;
    EXPECT(devbuf_grow_keep(b, 8, 20, copy_fails, &grew) == MC_ERR_HIP && !grew && b.get() == p && b.capacity() == 9 &&
           counts_up(b, 8) && live(72, 1));   // the new block went back
    EXPECT(devbuf_grow_keep(b, 10, 20, copy_ok) == MC_ERR_STATE && b.get() == p);   // more kept than held
  }
  EXPECT(live(0, 0));
  std::printf("bad %d\n", bad);
  return bad ? 1 : 0;
}
