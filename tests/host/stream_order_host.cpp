// The kernels' unit orders (csrc/unit_order.hpp: xcd_unit, stream_unit) compiled for the CPU, for
// tests/test_stream_order.py: stream_unit is a bijection on [0, n) for every order and n <= 3000, and each
// order starts where the order it answers ended.  Prints "bad <count>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "unit_order.hpp"
using namespace mc;

int main() {
  long bad = 0;
  for (int64_t n = 1; n <= 3000; ++n) {
    for (int order = 0; order < 4; ++order) {
      std::vector<char> seen(n, 0);
      for (int64_t b = 0; b < n; ++b) {
        const int64_t u = stream_unit(order, b, n);
        if (u < 0 || u >= n || seen[u]) { ++bad; break; }
        seen[u] = 1;
      }
    }
    for (int64_t b = 0; b < n; ++b) {
      if (stream_unit(0, b, n) != b) ++bad;
      if (stream_unit(1, b, n) != n - 1 - b) ++bad;
      if (stream_unit(2, b, n) != xcd_unit<true>(b, n)) ++bad;
    }
    // order 3 runs each XCD range of order 2 backwards: the units order 2 reaches last come first
    for (int64_t b = 0; b < n && b < kXcds; ++b) {
      const int64_t x = b % kXcds, per = n / kXcds, rem = n % kXcds;
      const int64_t len = per + (x < rem ? 1 : 0);
      if (len == 0) continue;
      if (stream_unit(3, b, n) != xcd_unit<true>(b + kXcds * (len - 1), n)) ++bad;
    }
  }
  std::printf("bad %ld\n", bad);
  return bad != 0;
}
