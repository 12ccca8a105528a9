// ingest_token_core.hpp — the text token parser of the ingest decoders (ingest.hpp): ingest_token / ingest_line.
// A core header (DESIGN.md "Core headers"): the device compiles this text and so does tests/host/ingest_host.cpp.
// Needs no stand-in.  No HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

// ---- the text token parser --------------------------------------------------------------------------------
// Grammar: [+-]?digits[.digits*] | nan | [+-]?inf.  With the sign, the leading zeros and the
// fraction's trailing zeros stripped the token is M / 10^k, M an integer of nsig significant digits.
// Inside the window nsig <= 19 (M < 10^19 < 2^64), k <= 19 the float64 is strtod's, bit for bit:
//   M < 2^53         M and 10^k (k <= 22) are exact float64s, one IEEE division rounds M / 10^k once
//   k == 0           the integer conversion rounds M once
//   otherwise        Q = floor(M 2^s / 10^k) with 55 or 56 bits and the remainder as a sticky bit,
//                    rounded half-to-even to 53 bits, scaled by 2^-s (exact: no subnormals here)
// Everything else (an exponent, more digits, other text) is "beyond the device parser": bad = 1 and
// no value.
struct IngestTok {
  double v;
  int bad;   // 1: beyond the parser
  int len;   // bytes up to the separator / end of line
};

MC_CORE_DEV double ingest_p10(int k) {
  static constexpr double T[20] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,
                                   1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19};
  return T[k];
}
MC_CORE_DEV uint64_t ingest_p10u(int k) {
  static constexpr uint64_t T[20] = {1ull,
                                     10ull,
                                     100ull,
                                     1000ull,
                                     10000ull,
                                     100000ull,
                                     1000000ull,
                                     10000000ull,
                                     100000000ull,
                                     1000000000ull,
                                     10000000000ull,
                                     100000000000ull,
                                     1000000000000ull,
                                     10000000000000ull,
                                     100000000000000ull,
                                     1000000000000000ull,
                                     10000000000000000ull,
                                     100000000000000000ull,
                                     1000000000000000000ull,
                                     10000000000000000000ull};
  return T[k];
}

// M / 10^k correctly rounded, 2^53 <= M < 2^64, 1 <= k <= 19
MC_CORE_DEV double ingest_div(uint64_t M, int k) {
  const uint64_t D = ingest_p10u(k);
  const int bm = 64 - __builtin_clzll(M), bd = 64 - __builtin_clzll(D);
  const int s = 55 - bm + bd;   // floor(M 2^s / D) lies in [2^54, 2^56)
  unsigned __int128 num = M, den = D;
  if (s >= 0) num <<= s; else den <<= -s;
  const unsigned __int128 Q = num / den;
  const bool sticky = num - Q * den != 0;
  const uint64_t q = (uint64_t)Q;
  const int sh = (64 - __builtin_clzll(q)) - 53;   // 2 or 3
  uint64_t mant = q >> sh;
  const uint64_t low = q & ((1ull << sh) - 1), half = 1ull << (sh - 1);
  if (low > half || (low == half && (sticky || (mant & 1)))) ++mant;
  return ldexp((double)mant, sh - s);
}

MC_CORE_DEV bool ingest_at_end(const char* q, const char* e, char sep) {
  return q >= e || *q == sep || *q == '\n' || *q == '\r';
}

// the token at p (the text ends at e); empty_nan: an empty token is NaN (pandas' na_rep, CSIM:1712)
MC_CORE_DEV IngestTok ingest_token(const char* p, const char* e, char sep, bool empty_nan) {
  IngestTok r;
  r.v = 0.0; r.bad = 0; r.len = 0;
  const char* q = p;
  if (ingest_at_end(q, e, sep)) {
    if (empty_nan) r.v = __builtin_nan(""); else r.bad = 1;
    return r;
  }
  bool neg = false, sign = false;
  if (*q == '-' || *q == '+') { neg = *q == '-'; sign = true; ++q; }
  bool ok = true, special = false;
  uint64_t M = 0;
  int nsig = 0, k = 0, pz = 0, nint = 0;
  if (e - q >= 3 && ((q[0] == 'n' && q[1] == 'a' && q[2] == 'n' && !sign) || (q[0] == 'i' && q[1] == 'n' && q[2] == 'f'))) {
    r.v = q[0] == 'n' ? __builtin_nan("") : __builtin_inf();
    special = true;
    q += 3;
  } else {
    while (!ingest_at_end(q, e, sep) && *q >= '0' && *q <= '9') {
      const uint32_t d = (uint32_t)(*q - '0');
      ++nint;
      if (M || d) {
        if (nsig < 19) M = M * 10 + d;
        ++nsig;
      }
      ++q;
    }
    if (nint == 0) ok = false;
    if (!ingest_at_end(q, e, sep) && *q == '.') {
      ++q;
      while (!ingest_at_end(q, e, sep) && *q >= '0' && *q <= '9') {
        const uint32_t d = (uint32_t)(*q - '0');
        if (d == 0) {
          ++pz;            // counts only once a later digit is not zero
        } else {
          if (M) nsig += pz;
          ++nsig;
          k += pz + 1;
          if (nsig <= 19 && k <= 19) M = (M ? M * ingest_p10u(pz) : 0) * 10 + d;
          pz = 0;
        }
        ++q;
      }
    }
  }
  while (!ingest_at_end(q, e, sep)) { ok = false; ++q; }
  r.len = (int)(q - p);
  if (!ok || nsig > 19 || k > 19) { r.bad = 1; r.v = 0.0; return r; }
  if (!special) {
    if (M < (1ull << 53)) r.v = (double)M / ingest_p10(k);
    else if (k == 0) r.v = (double)M;
    else r.v = ingest_div(M, k);
  }
  if (neg) r.v = -r.v;
  return r;
}

constexpr int kIngestMaxCols = 8;
constexpr int kIngestBadToken = 1, kIngestBadFields = 2, kIngestBadTime = 3;

// one line at p: n_cols fields into v; 0, kIngestBadToken or kIngestBadFields (the first fault from the left)
MC_CORE_DEV int ingest_line(const char* p, const char* e, char sep, int n_cols, bool empty_nan, double* v) {
  MC_CORE_UNROLL
  for (int k = 0; k < kIngestMaxCols; ++k) {
    if (k >= n_cols) break;
    const IngestTok t = ingest_token(p, e, sep, empty_nan);
    if (t.bad) return kIngestBadToken;
    v[k] = t.v;
    p += t.len;
    if (k + 1 < n_cols) {
      if (p < e && *p == sep) ++p; else return kIngestBadFields;
    }
  }
  if (p >= e || *p == '\n' || (*p == '\r' && (p + 1 >= e || p[1] == '\n'))) return 0;
  return kIngestBadFields;
}

}  // namespace mc
