// pcd_line_core.hpp — the packed "%.6f" line writer of the ASCII PCD kernels (codecs.hpp): pcd_fast,
// digit_groups, pcd_text, pcd_emit_line, pcd_fast_len and their float32 forms.  A core header (DESIGN.md "Core
// headers"): the device compiles this text and so does tests/host/pcd_formatter_host.cpp.  On the host it needs
// tests/host/device_standins.hpp (__umul24, __mul24, __builtin_amdgcn_perm, __hip_atomic_fetch_or, uint4, the
// std:: math names).  The row source and the packed 16-bit split are the including unit's: codecs.hpp defines
// them for the device, the harness for the host.  No HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

struct CodecFrames;
MC_CORE_DEV_DECL void codec_point(const CodecFrames& s, int32_t f, int64_t row, double c[4]);
MC_CORE_DEV_DECL void pk_tens_units(uint32_t v, uint32_t& t, uint32_t& u);

// ---- packed line path (every value of the line |v| < 4294, ties included) ----------------------
// The common LiDAR line is formatted from four 32-bit integers N = round(|v| * 10^6): the digits come
// out of 2-digit groups split with packed 16-bit arithmetic (digit_groups, value_fields), and each value
// goes to the tile's LDS text at its final byte offset (pcd_text, pcd_emit_line).  Tiles holding a line with
// any other value (NaN, inf, |v| >= 4294) take the byte path (fmt6_prepare / pcd_emit,
// k_pcd_write_bytes).  Rejected in round 4 (tools/ab_codecs.py --source batch, profiles/round4/s07,
// measure + write): digits from a 200-byte "00".."99" LDS pair table, 909.4 vs 872.6 us (fewer VALU
// instructions, but five dependent LDS reads per value with bank conflicts); each value's text as
// unaligned 8-byte LDS stores with exact line boundaries, 1084.2 us.
struct PcdFast {
  uint32_t n[4];   // round-half-even(|v| * 10^6)
  uint32_t ip[4];  // n / 10^6 (the integer part)
  uint32_t neg;    // bit k: value k is negative (signbit)
  bool ok;         // all four values took the fast path
};

// floor(N / 10^6) for N < 2^32 given as an exact float64: N 10^-6 is within 5e-13 of N / 10^6,
// whose fraction is 0 or at least 10^-6 from 1, so adding 10^-9 and truncating is exact (one
// full-rate f64 FMA + convert instead of the quarter-rate 32-bit mul_hi of N / 10^6)
// (against N / 10^6 on the integers: measure + write 812.4 vs 818.0 us, profiles/round4/s15 — within
// noise, kept for the four quarter-rate multiplies per line it removes)
MC_CORE_DEV uint32_t fast_ip(double N) { return (uint32_t)fma(N, 1e-6, 1e-9); }

// N = round-half-even(|v| * 10^6) exactly, for |v| < 4294 (NaN / larger values fail the test).
// y = fl(a * 10^6) and e = fma(a, 10^6, -y) represent the exact product as y + e; fr = y - floor(y)
// and fr - 0.5 are exact, so d = (fr - 0.5) + e has the sign of the exact fraction minus one half
// (rounding preserves signs) and is zero only on an exact tie, which rounds to even.  Exact ties are
// common in float32-valued clouds (any odd multiple of 1/128).
MC_CORE_DEV bool fmt6_fast(double v, uint32_t& n, uint32_t& ip) {
  const double a = fmin(fabs(v), 4294.0);
  const double y = a * 1000000.0;
  const double e = fma(a, 1000000.0, -y);
  const double fl = floor(y);
  const double d = ((y - fl) - 0.5) + e;
  const uint32_t m = (uint32_t)fl;
  n = m + ((d > 0.0 || (d == 0.0 && (m & 1u))) ? 1u : 0u);
  ip = fast_ip((double)n);
  return fabs(v) < 4294.0;
}

MC_CORE_DEV void pcd_fast(const CodecFrames& s, int32_t f, int64_t row, PcdFast& P) {
  double c[4];
  codec_point(s, f, row, c);
  P.ok = true;
  P.neg = 0;
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    P.ok &= fmt6_fast(c[k], P.n[k], P.ip[k]);
    P.neg |= (signbit(c[k]) ? 1u : 0u) << k;
  }
}

// ---- float32 source (a batch's own columns) ----------------------------------------------------
// v = m 2^e with a 24-bit m: |v| 10^6 = m 10^6 2^e has a significand below 2^44, so the float64
// product is exact and N = rint(|v| 10^6) (round half to even) is exact with no error term.
MC_CORE_DEV bool fmt6_fast_f32(float v, uint32_t& n, uint32_t& ip) {
  const float a = fminf(fabsf(v), 4294.0f);   // NaN -> 4294 (the line fails the test below)
  const double y = rint((double)a * 1000000.0);
  n = (uint32_t)y;
  ip = fast_ip(y);
  return fabsf(v) < 4294.0f;
}

MC_CORE_DEV void pcd_fast_vals_f32(const float c[4], PcdFast& P) {
  P.ok = true;
  P.neg = 0;
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    P.ok &= fmt6_fast_f32(c[k], P.n[k], P.ip[k]);
    P.neg |= (signbit(c[k]) ? 1u : 0u) << k;
  }
}

// pcd_fast_vals_f32 for a tile the measure pass found packed (every value |v| < 4294): no clamp and
// no path test (a NaN cannot reach here; it would convert to 0)
MC_CORE_DEV void pcd_fast_vals_packed(const float c[4], PcdFast& P) {
  P.ok = true;
  P.neg = 0;
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double y = rint((double)fabsf(c[k]) * 1000000.0);
    P.n[k] = (uint32_t)y;
    P.ip[k] = fast_ip(y);
    P.neg |= (signbit(c[k]) ? 1u : 0u) << k;
  }
}

// pcd_fast_len for float32 values: line length, or -1 outside the packed path
MC_CORE_DEV int pcd_fast_len_f32(const float c[4]) {
  int len = 4 + 4 * 8;
  bool ok = true;
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    const float a = fabsf(c[k]);
    ok = ok && a < 4294.0f;
    len += (signbit(c[k]) ? 1 : 0) + (a >= 10.0f) + (a >= 100.0f) + (a >= 1000.0f);
  }
  return ok ? len : -1;
}

// Digit groups of N = round(|v| 10^6) < 2^32 (|v| < 4294, so ip = N / 10^6 < 2^13): the ten digits
// as five 2-digit groups, g0 = ip / 100, g1 = ip % 100, g2 = fp / 10^4, g3 = fp / 100 % 100 and
// g4 = fp % 100 (fp = N - 10^6 ip), returned as g01 = g0 | g1 << 16, g23 = g2 | g3 << 16 and g4 (two
// values' g4 are split together, pair_tu4).  g2 = (fp 429497) >> 32 is fp / 10^4 exactly for
// fp < 10^6 (the multiplier's excess adds < 6.3e-5 to a quotient whose fraction is at most 0.9999).
// The products are 24-bit multiply-adds (v_mad_i32_i24 by __mul24 with a negative constant, no
// range masks).  Against the two 3-digit halves in 32-bit SWAR: 802.8 vs 806.8 us measure + write
// (profiles/round4/s17).
MC_CORE_DEV void digit_groups(uint32_t N, uint32_t ip, uint32_t& g01, uint32_t& g23, uint32_t& g4) {
  const uint32_t fp = N + (uint32_t)__mul24((int)ip, -1000000);                         // < 10^6
  uint32_t g2 = (uint32_t)(((uint64_t)(fp & 0xFFFFFu) * 429497ull) >> 32);             // fp / 10^4
  // opaque to the optimiser: it recognises fp - (fp / 10^4) 10^4 as fp % 10^4 and lowers that
  // through a quarter-rate 64-bit multiply-add
  asm("" : "+v"(g2));
  const uint32_t r4 = fp + (uint32_t)__mul24((int)g2, -10000);                          // < 10^4
  const uint32_t g3 = __umul24(r4, 5243u) >> 19;                                        // r4 / 100
  g4 = r4 - g3 * 100u;
  const uint32_t g0 = __umul24(ip, 5243u) >> 19;                                        // ip / 100
  const uint32_t g1 = ip - g0 * 100u;
  g01 = g0 | (g1 << 16);
  g23 = g2 | (g3 << 16);
}
// tens | units << 8 of two values' g4 at once (one packed split for both)
MC_CORE_DEV void pair_tu4(uint32_t ga, uint32_t gb, uint32_t& tua, uint32_t& tub) {
  uint32_t T, U;
  pk_tens_units(ga | (gb << 16), T, U);
  tua = __builtin_amdgcn_perm(U, T, 0x0C0C0400u);
  tub = __builtin_amdgcn_perm(U, T, 0x0C0C0602u);
}
// Text fields of one value (bytes in text order, v_perm_b32 placement): D = the 4 integer digits
// with leading zeros as values 0..9 (byte 0 = thousands), A = ". d1 d2 d3", B = "d4 d5 d6 sep"
MC_CORE_DEV void value_fields(uint32_t g01, uint32_t g23, uint32_t tu4, uint32_t sep, uint32_t& D,
                                             uint32_t& A, uint32_t& B) {
  uint32_t T1, U1, T2, U2;
  pk_tens_units(g01, T1, U1);
  pk_tens_units(g23, T2, U2);
  D = __builtin_amdgcn_perm(T1, U1, 0x02060004u);
  A = __builtin_amdgcn_perm(T2, U2, 0x0600040Cu) + 0x3030302Eu;
  B = __builtin_amdgcn_perm(U2, tu4, 0x0C010006u) + (0x00303030u | (sep << 24));
}
MC_CORE_DEV void put4(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// A packed line's text: value k's fields D (ASCII), A, B, its count q of leading zero digits in D
// (4 - its integer digit count: the index of D's first non-zero digit byte, one v_ffbl_b32), the sign
// bits and the line length 4 (nd + [v < 0] + 8) summed = 48 + sum([v < 0] - q).  The digit count
// comes out of the digits themselves, so it is N >= 10^7 / 10^8 / 10^9 exactly (no compares).
struct PcdText {
  uint32_t D[4], A[4], B[4];
  int q0;      // q of value 0
  int ng[4];   // 1: value k is negative
  int d[4];    // ng - q: value k's text is 12 + d[k] bytes with its separator
  int len;
};
MC_CORE_DEV void pcd_text(const PcdFast& P, PcdText& T) {
  uint32_t g01[4], g23[4], g4[4], tu4[4];
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) digit_groups(P.n[k], P.ip[k], g01[k], g23[k], g4[k]);
  pair_tu4(g4[0], g4[1], tu4[0], tu4[1]);
  pair_tu4(g4[2], g4[3], tu4[2], tu4[3]);
  int len = 48;
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    uint32_t D;
    value_fields(g01[k], g23[k], tu4[k], k == 3 ? '\n' : ' ', D, T.A[k], T.B[k]);
    const int q = (int)(__builtin_ctz(D | 0x01000000u) >> 3);   // the units byte always counts
    if (k == 0) T.q0 = q;
    T.D[k] = D + 0x30303030u;
    T.ng[k] = (int)((P.neg >> k) & 1u);
    T.d[k] = T.ng[k] - q;
    len += T.d[k];
  }
  T.len = len;
}

// One packed line at byte `off` of the tile text, OR-ed into the zeroed text buffer (pcd_tile_text) as
// naturally aligned 8-byte words: value k's 16 bytes [pa - 8, pa + 8) — H = the 8 bytes ending at its
// '.' (zeros, its '-' if negative, its integer digits with the leading zeros blanked), then A, B —
// shifted to the 8-byte grid are three ds_or_b64 whose zero bytes leave the neighbours' text (the
// line's other values, other lanes' lines) untouched.  Naturally aligned LDS stores issue at 4.6
// ticks per wave-instruction, the unaligned 8 / 12-byte stores of byte-offset text at 36
// (tools/issue_probe.hip, profiles/round5/s02); against those stores (values 3..1 as unaligned
// 12-byte fields overwriting each other's heads, value 0 byte by byte): measure + write 772.1 / 782.5
// vs 788.7 / 793.5 us, fused write pass 630.9 / 635.2 vs 639.8 / 642.7 us (profiles/round5/s03, s04;
// ds_or_b32 on 4-byte words ran alike but took more VALU).  base is 16 bytes into the buffer (value
// 0's window starts up to 7 bytes before its line).
typedef __attribute__((address_space(3))) uint64_t lds_u64;
MC_CORE_DEV void lds_or64(uint8_t* p, uint64_t v) {
  __hip_atomic_fetch_or((lds_u64*)(void*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// one value whose '.' is at byte pa: D its 4 integer digit characters, q of them leading zeros, ng 1
// if negative
MC_CORE_DEV void pcd_emit_value(uint8_t* base, int pa, uint32_t D, uint32_t A, uint32_t B, int q,
                                               int ng) {
  const uint32_t Dm = D & (0xFFFFFFFFu << (8 * q));
  const uint64_t H = ((uint64_t)Dm << 32) | ((uint64_t)(ng ? 0x2Du : 0u) << (24 + 8 * q));
  const uint64_t AB = ((uint64_t)B << 32) | A;
  const int s0 = pa - 8, r = s0 & 7;
  uint8_t* const w = base + (s0 - r);   // 8-byte aligned
  const int sh = 8 * r;                 // 0 .. 56
  // x >> (64 - sh) as (x >> 8) >> (56 - sh): zero at sh = 0 (one 64-bit shift takes its amount mod 64)
  lds_or64(w, H << sh);
  lds_or64(w + 8, (AB << sh) | ((H >> 8) >> (56 - sh)));
  lds_or64(w + 16, (AB >> 8) >> (56 - sh));
}
// text: the tile's text buffer as 16-byte chunks — typed uint4 so the 8-byte grid pcd_emit_value
// ORs into is the buffer's own alignment (a ds_or_b64 at a 4-byte LDS offset faults, profiles/round5/s03)
MC_CORE_DEV void pcd_emit_line(const PcdText& T, uint4* text, int off) {
  static_assert(alignof(uint4) % 8 == 0, "the text chunks must keep the 8-byte grid of ds_or_b64");
  uint8_t* const base = reinterpret_cast<uint8_t*>(text);
  int pa = off + 4 + T.d[0];   // the '.' of value k
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    if (k > 0) pa += 12 + T.d[k];
    pcd_emit_value(base, pa, T.D[k], T.A[k], T.B[k], T.ng[k] - T.d[k], T.ng[k]);
  }
}

// The packed line's length without its digits: "%.6f" of |v| < 4294 has 1 + [v < 0] + nd + 7
// characters with the separator, nd = 1 + [N >= 10^7] + [N >= 10^8] + [N >= 10^9] for
// N = round-half-even(|v| 10^6).  N >= T (T even) <=> |v| 10^6 >= T - 1/2 exactly; y = fl(|v| 10^6)
// decides that except when y lands on T - 1/2, where the product's error e does.  -1: a value
// outside the packed path.
MC_CORE_DEV int pcd_fast_len(const double c[4]) {
  int len = 4 + 4 * 8;
  bool ok = true;
  MC_CORE_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double a = fabs(c[k]);
    ok = ok && a < 4294.0;
    const double y = a * 1000000.0;
    const bool tie_up = fma(a, 1000000.0, -y) >= 0.0;
    len += (signbit(c[k]) ? 1 : 0) + (y > 9999999.5 || (y == 9999999.5 && tie_up)) +
           (y > 99999999.5 || (y == 99999999.5 && tie_up)) + (y > 999999999.5 || (y == 999999999.5 && tie_up));
  }
  return ok ? len : -1;
}

}  // namespace mc
