// devbuf_host.cpp — csrc/devbuf.hpp on the host (MC_DEVBUF_HOST_TEST: malloc / free behind the seam,
// an allocation above g_test_fail_above bytes fails), built under ASan + UBSan + leak detection by
// tests/test_sanitizers.py.  Prints "bad <n>"; exit status 1 when n > 0.
#include "devbuf.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>

namespace mcimpl {
int fail(int code, const char*, ...) { return code; }
}  // namespace mcimpl
using mcimpl::DevBuf;
using mcimpl::g_live_blocks;
using mcimpl::g_live_bytes;
using mcimpl::g_test_fail_above;

static int bad = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) { ++bad; std::printf("line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static bool live(int64_t bytes, int64_t blocks) { return g_live_bytes == bytes && g_live_blocks == blocks; }
// every element of the block is the caller's to write (ASan checks the extent)
template <typename T, int W>
static void fill(const DevBuf<T, W>& b) { std::memset(b.get(), 0x5A, b.capacity() * sizeof(T)); }

struct Three {
  DevBuf<double> a;
  DevBuf<int32_t> b;
  DevBuf<char> c;
  int build(size_t n) {
    if (int r = a.alloc(n)) return r;
    if (int r = b.alloc(n)) return r;
    if (int r = c.alloc(4096)) return r;
    return MC_OK;
  }
};

int main() {
  {  // empty; alloc(0) is one element
    DevBuf<double> b;
    EXPECT(!b && b.get() == nullptr && b.capacity() == 0 && live(0, 0));
    EXPECT(b.alloc(0) == MC_OK && b && b.capacity() == 1 && live(8, 1));
    fill(b);
    EXPECT(b.alloc(5) == MC_OK && b.capacity() == 5 && live(40, 1));   // the old block went back
    fill(b);
  }
  EXPECT(live(0, 0));
  {  // reserve below, at and above the capacity
    DevBuf<int32_t> b;
    bool grew = true;
    EXPECT(b.reserve(0, &grew) == MC_OK && !grew && !b && live(0, 0));
    EXPECT(b.reserve(10, &grew) == MC_OK && grew && b.capacity() == 10 && live(40, 1));
    int32_t* p = b;
    EXPECT(b.reserve(3, &grew) == MC_OK && !grew && b.get() == p && b.capacity() == 10);
    EXPECT(b.reserve(10, &grew) == MC_OK && !grew && b.get() == p && live(40, 1));
    EXPECT(b.reserve(11, &grew) == MC_OK && grew && b.capacity() == 11 && live(44, 1));
    fill(b);
    EXPECT(b.reserve(11) == MC_OK && b.capacity() == 11);   // grew is optional
    EXPECT(b.as<char>() == reinterpret_cast<char*>(b.get()));
  }
  EXPECT(live(0, 0));
  {  // an injected failure leaves the buffer empty, whatever it held
    DevBuf<double> b;
    g_test_fail_above = 64;
    EXPECT(b.alloc(9) == MC_ERR_NOMEM && !b && b.capacity() == 0 && live(0, 0));
    EXPECT(b.alloc(8) == MC_OK && live(64, 1));
    bool grew = true;
    EXPECT(b.reserve(9, &grew) == MC_ERR_NOMEM && !grew && !b && b.capacity() == 0 && live(0, 0));
    EXPECT(b.reserve(8, &grew) == MC_OK && grew && live(64, 1));
    EXPECT(b.alloc(100) == MC_ERR_NOMEM && !b && live(0, 0));
    g_test_fail_above = SIZE_MAX;
  }
  EXPECT(live(0, 0));
  {  // moves: onto an empty and onto a full buffer; the source is left empty
    DevBuf<double> a;
    EXPECT(a.alloc(4) == MC_OK);
    double* pa = a;
    DevBuf<double> b(std::move(a));
    EXPECT(!a && a.capacity() == 0 && b.get() == pa && b.capacity() == 4 && live(32, 1));
    DevBuf<double> c;
    c = std::move(b);   // onto an empty one
    EXPECT(!b && c.get() == pa && live(32, 1));
    DevBuf<double> d;
    EXPECT(d.alloc(6) == MC_OK && live(80, 2));
    d = std::move(c);   // onto a full one: its block goes back
    EXPECT(!c && d.get() == pa && d.capacity() == 4 && live(32, 1));
    DevBuf<double>& self = d;
    d = std::move(self);
    EXPECT(d.get() == pa && live(32, 1));
    d = DevBuf<double>();   // an empty source empties the target
    EXPECT(!d && live(0, 0));
  }
  EXPECT(live(0, 0));
  {  // reset twice
    DevBuf<char> b;
    EXPECT(b.alloc(100) == MC_OK && live(100, 1));
    b.reset();
    EXPECT(!b && b.capacity() == 0 && live(0, 0));
    b.reset();
    EXPECT(!b && live(0, 0));
  }
  {  // a handle of several buffers whose third allocation fails: the first two go with it
    g_test_fail_above = 4000;
    {
      Three t;
      EXPECT(t.build(16) == MC_ERR_NOMEM && t.a && t.b && !t.c && live(16 * 8 + 16 * 4, 2));
    }
    EXPECT(live(0, 0));
    g_test_fail_above = SIZE_MAX;
    Three ok;
    EXPECT(ok.build(16) == MC_OK && live(16 * 8 + 16 * 4 + 4096, 3));
  }
  {  // pinned host blocks are not in the account
    mcimpl::PinBuf<char, 0u> p;
    EXPECT(p.alloc(64) == MC_OK && p && live(0, 0));
    fill(p);
    EXPECT(p.reserve(128) == MC_OK && p.capacity() == 128 && live(0, 0));
  }
  EXPECT(live(0, 0));
  std::printf("bad %d\n", bad);
  return bad ? 1 : 0;
}
