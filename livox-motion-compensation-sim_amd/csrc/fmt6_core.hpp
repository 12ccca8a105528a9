// fmt6_core.hpp — the exact "%.6f" formatter of the text writers (codecs.hpp, csim_codecs.hpp): fmt6_prepare /
// fmt6_write.  A core header (DESIGN.md "Core headers"): the device compiles this text and so does
// tests/host/csim_text_host.cpp.  On the host it needs tests/host/device_standins.hpp (__double_as_longlong,
// __umul24, the std:: math names).  No HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

// ---- "%.6f" (Python's correctly rounded fixed-point float formatting) -------------------------
// v = m * 2^e exactly; N = round-half-even(|v| * 10^6) in 128-bit integer arithmetic, printed as
// ip = N / 10^6, "." and the six digits of N % 10^6.  |v| < 2^107 (~1.6e32) is supported; larger
// values set the error flag.  |v| < 4294.97 (N < 2^32, every LiDAR coordinate) stays in 32-bit
// integer arithmetic.
struct Fmt6 {
  unsigned __int128 ip;
  uint32_t fp;
  int nd;      // digits of ip
  int len;     // characters
  int kind;    // 0 finite, 1 inf, 2 nan, 3 out of range
  bool neg;
};

MC_CORE_DEV int u32_digits(uint32_t x) {
  return 1 + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) +
         (x >= 10000000u) + (x >= 100000000u) + (x >= 1000000000u);
}

MC_CORE_DEV_NOINLINE Fmt6 fmt6_prepare_exact(double v);

// Common case, |v| < 4294: y = |v| * 1e6 in double is within 2.4e-7 of the exact product, so
// unless y's fraction is within 1e-6 of one half the rounded integer is floor(y) or floor(y) + 1
// as decided by the fraction — no 128-bit arithmetic.  Otherwise (and for NaN / inf / large
// magnitudes) the exact path decides.
MC_CORE_DEV Fmt6 fmt6_prepare(double v) {
  const double a = fabs(v);
  if (a < 4294.0) {
    const double y = a * 1000000.0;
    const double fl = floor(y);
    const double fr = y - fl;
    if (fabs(fr - 0.5) > 1e-6) {
      Fmt6 r;
      const uint32_t n = (uint32_t)fl + (fr > 0.5 ? 1u : 0u);
      const uint32_t ip = n / 1000000u;
      r.neg = signbit(v);
      r.kind = 0;
      r.ip = ip;
      r.fp = n - ip * 1000000u;
      r.nd = 1 + (ip >= 10u) + (ip >= 100u) + (ip >= 1000u);
      r.len = (r.neg ? 1 : 0) + r.nd + 7;
      return r;
    }
  }
  return fmt6_prepare_exact(v);
}

MC_CORE_DEV_NOINLINE Fmt6 fmt6_prepare_exact(double v) {
  Fmt6 r;
  const uint64_t bits = (uint64_t)__double_as_longlong(v);
  r.neg = (bits >> 63) != 0;
  const int ex = (int)((bits >> 52) & 0x7ff);
  const uint64_t frac = bits & ((1ull << 52) - 1);
  r.ip = 0; r.fp = 0; r.nd = 1;
  if (ex == 0x7ff) {                                // "nan" (Python drops a NaN's sign) / "inf" / "-inf"
    r.kind = frac ? 2 : 1;
    r.len = 3 + (r.kind == 1 && r.neg ? 1 : 0);
    return r;
  }
  const uint64_t m = ex ? (frac | (1ull << 52)) : frac;
  const int e = ex ? ex - 1075 : -1074;
  const unsigned __int128 P = (unsigned __int128)m * 1000000u;   // < 2^73
  unsigned __int128 N = 0;
  if (e >= 0) {
    if (e > 54) { r.kind = 3; r.len = 0; return r; }
    N = P << e;
  } else if (-e < 74) {
    const int s = -e;
    const unsigned __int128 one = 1;
    unsigned __int128 q = P >> s;
    const unsigned __int128 rem = P & ((one << s) - 1);
    const unsigned __int128 half = one << (s - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    N = q;
  }
  r.kind = 0;
  // e < 0: only then can N be below 2^32, and N < 2^73 there, so the 64-bit view of N >> 32 is all of
  // it.  Without it 2^100 (N = 2^106 5^6, bits 32..95 zero) printed "0.000000", as did every
  // float32-valued |v| >= 2^90 with enough trailing zero bits.
  if (e < 0 && (uint64_t)(N >> 32) == 0) {
    const uint32_t n = (uint32_t)N;
    const uint32_t ip = n / 1000000u;
    r.ip = ip;
    r.fp = n - ip * 1000000u;
    r.nd = u32_digits(ip);
  } else {
    const unsigned __int128 ip = (uint64_t)(N >> 64) == 0 ? (unsigned __int128)((uint64_t)N / 1000000u)
                                                          : N / 1000000u;
    r.ip = ip;
    r.fp = (uint32_t)(N - ip * 1000000u);
    int d = 1;
    for (unsigned __int128 x = ip; x >= 10; x /= 10) ++d;
    r.nd = d;
  }
  r.len = (r.neg ? 1 : 0) + r.nd + 7;
  return r;
}

// the last min(n, 3) decimal digits of x < 1000 at q[3-n .. 2] (q[0..2] = hundreds, tens, units)
MC_CORE_DEV void put3(char* q, uint32_t x, int n) {
  const uint32_t h = __umul24(x, 41u) >> 12;
  const uint32_t r = x - h * 100u;
  const uint32_t t = __umul24(r, 103u) >> 10;
  if (n >= 3) q[0] = (char)('0' + h);
  if (n >= 2) q[1] = (char)('0' + t);
  q[2] = (char)('0' + (r - t * 10u));
}

// writes f.len characters at p (generic pointer: LDS or global)
MC_CORE_DEV void fmt6_write(const Fmt6& f, char* p) {
  if (f.kind == 3) return;
  if (f.kind == 2) { p[0] = 'n'; p[1] = 'a'; p[2] = 'n'; return; }
  if (f.neg) *p++ = '-';
  if (f.kind == 1) { p[0] = 'i'; p[1] = 'n'; p[2] = 'f'; return; }
  const int nd = f.nd;
  if (nd <= 4) {
    // ip < 10^4: 24-bit multiply-shift digit extraction ((x*41)>>12 == x/100 for x < 1000,
    // (x*103)>>10 == x/10 for x < 100, (x*8389)>>23 == x/1000 for x < 10^4)
    const uint32_t ip = (uint32_t)f.ip;
    const uint32_t th = __umul24(ip, 8389u) >> 23;
    put3(p + nd - 3, ip - th * 1000u, nd);
    if (nd == 4) p[0] = (char)('0' + th);
    p[nd] = '.';
    const uint32_t fh = f.fp / 1000u;
    put3(p + nd + 1, fh, 3);
    put3(p + nd + 4, f.fp - fh * 1000u, 3);
    return;
  }
  uint32_t fp = f.fp;
  MC_CORE_UNROLL
  for (int i = 6; i >= 1; --i) {
    const uint32_t q = fp / 10u;
    p[nd + i] = (char)('0' + (fp - q * 10u));
    fp = q;
  }
  p[nd] = '.';
  if (nd <= 10 && (uint64_t)(f.ip >> 32) == 0) {   // nd: the 64-bit view misses bits 96.. (2^100: bits 32..95 zero)
    uint32_t y = (uint32_t)f.ip;
    for (int i = nd - 1; i >= 0; --i) {
      const uint32_t q = y / 10u;
      p[i] = (char)('0' + (y - q * 10u));
      y = q;
    }
  } else {
    unsigned __int128 y = f.ip;
    for (int i = nd - 1; i >= 0; --i) { p[i] = (char)('0' + (uint32_t)(y % 10)); y /= 10; }
  }
}

}  // namespace mc
