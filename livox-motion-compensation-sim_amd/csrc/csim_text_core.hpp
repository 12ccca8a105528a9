// csim_text_core.hpp — the text formatters of the CSIM exports (csim_codecs.hpp): "%.0f" (fmt0_prepare /
// fmt0_write), the lines' "%.6f" (csim_fmt6_prepare / csim_fmt6_write) and a line's prepare / emit.  A core
// header (DESIGN.md "Core headers"): the device compiles this text and so does tests/host/csim_text_host.cpp.
// On the host it needs tests/host/device_standins.hpp (as fmt6_core.hpp).  No HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"
#include "fmt6_core.hpp"

namespace mc {

// ---- text --------------------------------------------------------------------------------------
// "%.0f" (Python's correctly rounded formatting): N = round-half-even(|v|) on the exact binary value
// (0.5 -> 0, 1.5 -> 2, 2.5 -> 2), the sign kept when N = 0 (-0.3 -> "-0"), "nan" / "inf" / "-inf".
// The same range as "%.6f": |v| < 2^107, larger values are kind 3.  The result reuses Fmt6 with
// ip = N and no fraction: len = [v < 0] + nd.
// Nanosecond timestamps (~1.7e18) are the one column far beyond 32 bits: their digits are counted
// with compares and written in 9-digit groups of 32-bit arithmetic, and their "%.6f" avoids the
// 128-bit products of fmt6_prepare_exact (csim_fmt6_prepare) — with 128-bit divisions per digit the
// CSV pass took 73 ms for 60 M lines instead of 3.
MC_CORE_DEV int u64_digits(uint64_t x) {
  if ((x >> 32) == 0) return u32_digits((uint32_t)x);
  int d = 10;                      // x >= 2^32 > 10^9
  uint64_t p = 10000000000ull;     // 10^10 .. 10^19 (10^19 < 2^64)
  MC_CORE_UNROLL
  for (int k = 10; k < 20; ++k) {
    d += x >= p ? 1 : 0;
    if (k < 19) p *= 10;
  }
  return d;
}

// the n <= 9 low decimal digits of y at p[0 .. n), leading zeros included
MC_CORE_DEV void put_u32(char* p, uint32_t y, int n) {
  for (int i = n - 1; i >= 0; --i) {
    const uint32_t q = y / 10u;
    p[i] = (char)('0' + (y - q * 10u));
    y = q;
  }
}

MC_CORE_DEV Fmt6 fmt0_prepare(double v) {
  Fmt6 r;
  const uint64_t bits = (uint64_t)__double_as_longlong(v);
  r.neg = (bits >> 63) != 0;
  const int ex = (int)((bits >> 52) & 0x7ff);
  const uint64_t frac = bits & ((1ull << 52) - 1);
  r.ip = 0; r.fp = 0; r.nd = 1;
  if (ex == 0x7ff) {
    r.kind = frac ? 2 : 1;
    r.len = 3 + (r.kind == 1 && r.neg ? 1 : 0);
    return r;
  }
  const uint64_t m = ex ? (frac | (1ull << 52)) : frac;
  const int e = ex ? ex - 1075 : -1074;
  r.kind = 0;
  if (e >= 0) {
    if (e > 54) { r.kind = 3; r.len = 0; return r; }
    r.ip = (unsigned __int128)m << e;
  } else if (-e <= 53) {             // (-e > 53: |v| < 1/2, N = 0)
    const int s = -e;
    uint64_t q = m >> s;
    const uint64_t rem = m & ((1ull << s) - 1), half = 1ull << (s - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    r.ip = q;
  }
  if (e < 0 && (uint64_t)(r.ip >> 32) == 0) {   // e >= 0: ip >= 2^52, and 2^100 (bits 32..95 zero) printed "6"
    r.nd = u32_digits((uint32_t)r.ip);
  } else if ((uint64_t)(r.ip >> 64) == 0) {
    r.nd = u64_digits((uint64_t)r.ip);
  } else {
    int d = 1;
    for (unsigned __int128 x = r.ip; x >= 10; x /= 10) ++d;
    r.nd = d;
  }
  r.len = (r.neg ? 1 : 0) + r.nd;
  return r;
}

// the nd decimal digits of x at p[0 .. nd)
MC_CORE_DEV void put_digits(char* p, unsigned __int128 x, int nd) {
  if ((uint64_t)(x >> 64) != 0) {
    for (int i = nd - 1; i >= 0; --i) { p[i] = (char)('0' + (uint32_t)(x % 10)); x /= 10; }
    return;
  }
  uint64_t y = (uint64_t)x;
  while (nd > 9) {                 // at most twice: nd <= 20
    const uint64_t q = y / 1000000000ull;
    put_u32(p + nd - 9, (uint32_t)(y - q * 1000000000ull), 9);
    y = q;
    nd -= 9;
  }
  put_u32(p, (uint32_t)y, nd);     // what is left has nd <= 9 digits
}

// "%.6f" for the lines here: fmt6_prepare, except that 4294 <= |v| < 2^64 (where fmt6_prepare goes
// through 128-bit arithmetic) splits v = I + r exactly, I = floor(|v|) and r = |v| - I in [0, 1), and
// rounds r 10^6 half-to-even as fmt6_fast does: y = fl(r 10^6) and e = fma(r, 10^6, -y) give the exact
// product y + e, (y - floor(y)) - 0.5 is exact, so d has the sign of the exact fraction minus one half
// and is zero only on an exact tie.  A fraction that rounds to 10^6 carries into I.  From 2^52 on
// every double is an integer.
MC_CORE_DEV Fmt6 csim_fmt6_prepare(double v) {
  const double a = fabs(v);
  if (!(a >= 4294.0 && a < 18446744073709551616.0)) return fmt6_prepare(v);   // also NaN
  Fmt6 r;
  const double I = floor(a);
  uint64_t ip = (uint64_t)I;
  uint32_t n = 0;
  if (a < 4503599627370496.0) {
    // y must be the rounded product in both of its uses: no fusing of fr * 10^6 into y - fl
    MC_CORE_NO_CONTRACT
    const double fr = a - I;
    const double y = fr * 1000000.0;
    const double e = fma(fr, 1000000.0, -y);
    const double fl = floor(y);
    const double d = ((y - fl) - 0.5) + e;
    const uint32_t m = (uint32_t)fl;
    n = m + ((d > 0.0 || (d == 0.0 && (m & 1u))) ? 1u : 0u);
    if (n == 1000000u) { n = 0; ++ip; }
  }
  r.neg = signbit(v);
  r.kind = 0;
  r.ip = ip;
  r.fp = n;
  r.nd = u64_digits(ip);
  r.len = (r.neg ? 1 : 0) + r.nd + 7;
  return r;
}

MC_CORE_DEV void csim_fmt6_write(const Fmt6& f, char* p) {
  if (f.kind != 0 || (uint64_t)(f.ip >> 32) == 0 || (uint64_t)(f.ip >> 64) != 0) { fmt6_write(f, p); return; }
  if (f.neg) *p++ = '-';
  put_digits(p, f.ip, f.nd);
  p[f.nd] = '.';
  put_u32(p + f.nd + 1, f.fp, 6);
}

// writes f.len characters at p (generic pointer: LDS or global)
MC_CORE_DEV void fmt0_write(const Fmt6& f, char* p) {
  if (f.kind == 3) return;
  if (f.kind == 2) { p[0] = 'n'; p[1] = 'a'; p[2] = 'n'; return; }
  if (f.neg) *p++ = '-';
  if (f.kind == 1) { p[0] = 'i'; p[1] = 'n'; p[2] = 'f'; return; }
  put_digits(p, f.ip, f.nd);
}

// A text line: ncols values (3 or 5) of columns 0 .. ncols - 1, `sep` between them and '\n' after the
// last; bit k of dec0 prints column k "%.0f", the others "%.6f"; nan_empty prints a NaN as an empty
// field (pandas' na_rep, CSIM:1712).
struct CsimLine {
  int32_t ncols;
  int32_t sep;
  uint32_t dec0;
  int32_t nan_empty;
};
constexpr int kCsimMaxCols = 5;
struct CsimText {
  Fmt6 v[kCsimMaxCols];
  int len;
};

MC_CORE_DEV void csim_line_prepare(const CsimLine& d, const double* c, CsimText& L, int* err) {
  L.len = d.ncols;                                   // the separators and the newline
  MC_CORE_UNROLL
  for (int k = 0; k < kCsimMaxCols; ++k) {
    if (k >= d.ncols) break;
    L.v[k] = ((d.dec0 >> k) & 1u) ? fmt0_prepare(c[k]) : csim_fmt6_prepare(c[k]);
    if (L.v[k].kind == 3) *err = 1;
    if (d.nan_empty && L.v[k].kind == 2) L.v[k].len = 0;
    L.len += L.v[k].len;
  }
}

MC_CORE_DEV void csim_line_emit(const CsimLine& d, const CsimText& L, char* p) {
  MC_CORE_UNROLL
  for (int k = 0; k < kCsimMaxCols; ++k) {
    if (k >= d.ncols) break;
    if (L.v[k].len) {
      if ((d.dec0 >> k) & 1u) fmt0_write(L.v[k], p);
      else csim_fmt6_write(L.v[k], p);
    }
    p += L.v[k].len;
    *p++ = k + 1 < d.ncols ? (char)d.sep : '\n';
  }
}

}  // namespace mc
