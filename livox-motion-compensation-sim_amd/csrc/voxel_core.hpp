// voxel_core.hpp — the scalar core of the voxel-grid filter (voxel.hpp), on plain values so the same
// text compiles for the device and for the host (tests/host/voxel_host.cpp includes it; built with
// g++ -ffp-contract=off).  A core header (DESIGN.md "Core headers"); needs no stand-in.  No HIP include.
//
// Every line of floating-point arithmetic is ONE IEEE float64 operation, never contracted:
//   a = double(v) - o     g = a / h     k = floor(g)     f = g - k   (f may round up to 1.0)
//   Q  = (int64) rint(f * 2^32)                    0 <= Q <= 2^32
//   QI = (int64) rint(double(intensity) * 2^16)
// A voxel (kx, ky, kz) keeps n, S[3] = sum Q and SI = sum QI as integers, so the sums do not depend
// on the order the points arrive in; its outputs are
//   m = double(S) / double(n)     w = double(k) + m * 2^-32     c = o + w * h
//   i = (double(SI) / double(n)) * 2^-16
// Bounds (include/mcdeskew.h): |c - mean| <= h * 2^-32 plus float64 rounding; the intensity
// is within 2^-17 of the mean.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

constexpr int32_t kVoxelKeyMin = -(1 << 20);      // keys in [-2^20, 2^20): 21 bits per axis
constexpr int32_t kVoxelKeyEnd = 1 << 20;
constexpr double kVoxelFrac = 4294967296.0;       // 2^32: the fixed point of a coordinate inside its voxel
constexpr double kVoxelFracInv = 1.0 / 4294967296.0;
constexpr double kVoxelInt = 65536.0;             // 2^16: the fixed point of the intensity
constexpr double kVoxelIntInv = 1.0 / 65536.0;
constexpr uint64_t kVoxelEmpty = ~0ull;           // a table slot without a key (bit 63 is never a key's)

struct VoxelPoint {
  int32_t k[3];
  int64_t Q[3];
  int64_t QI;
  int32_t bad;   // 1: refused (k, Q and QI are 0)
};

MC_CORE_HD bool voxel_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// one point: coordinates v (already float64), intensity, voxel size h > 0, origin o
MC_CORE_HD VoxelPoint voxel_quantise(const double v[3], double intensity, double h, const double o[3]) {
  MC_CORE_NO_CONTRACT
  VoxelPoint r;
  r.bad = 0;
  for (int c = 0; c < 3; ++c) {
    const double a = v[c] - o[c];
    const double g = a / h;
    const double k = floor(g);
    const double f = g - k;
    const bool ok = voxel_finite(v[c]) && voxel_finite(g) && k >= (double)kVoxelKeyMin && k < (double)kVoxelKeyEnd;
    r.k[c] = ok ? (int32_t)k : 0;
    r.Q[c] = ok ? (int64_t)rint(f * kVoxelFrac) : 0;
    if (!ok) r.bad = 1;
  }
  const bool iok = voxel_finite(intensity) && fabs(intensity) <= kVoxelInt;
  r.QI = iok ? (int64_t)rint(intensity * kVoxelInt) : 0;
  if (!iok) r.bad = 1;
  if (r.bad) {
    for (int c = 0; c < 3; ++c) { r.k[c] = 0; r.Q[c] = 0; }
    r.QI = 0;
  }
  return r;
}

// 63-bit key: 21 bits per axis, x highest; bit 63 stays clear (kVoxelEmpty has it set)
MC_CORE_HD uint64_t voxel_pack(const int32_t k[3]) {
  return ((uint64_t)(uint32_t)(k[0] - kVoxelKeyMin) << 42) | ((uint64_t)(uint32_t)(k[1] - kVoxelKeyMin) << 21) |
         (uint64_t)(uint32_t)(k[2] - kVoxelKeyMin);
}
MC_CORE_HD void voxel_unpack(uint64_t key, int32_t k[3]) {
  k[0] = (int32_t)((key >> 42) & 0x1FFFFFu) + kVoxelKeyMin;
  k[1] = (int32_t)((key >> 21) & 0x1FFFFFu) + kVoxelKeyMin;
  k[2] = (int32_t)(key & 0x1FFFFFu) + kVoxelKeyMin;
}

// The probe sequence of a key in a table of mask + 1 slots (a power of two, shift = 64 - log2 of it):
// Fibonacci hashing, then linear.  Slot index kVoxelNoSlot is never produced — it marks "no slot" in
// the per-point slot array, and a table of 2^32 slots (2^30 < N < 2^31 points) has a slot of that
// index; the sequence passes over it, leaving 2^32 - 1 >= 2 N usable slots.
constexpr uint32_t kVoxelNoSlot = 0xFFFFFFFFu;
MC_CORE_HD uint32_t voxel_slot_next(uint32_t at, uint32_t mask) {
  const uint32_t n = (at + 1u) & mask;
  return n == kVoxelNoSlot ? 0u : n;
}
MC_CORE_HD uint32_t voxel_slot_first(uint64_t key, int shift, uint32_t mask) {
  const uint32_t at = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift) & mask;
  return at == kVoxelNoSlot ? 0u : at;
}

// ---- growing a live cloud (voxel.hpp "insert into a live table") ------------------------------------
// A cloud holds fewer than 2^31 points in all: the uint32 count, the int32 emit and |S| < 2^63 stay safe.
constexpr int64_t kVoxelPointsEnd = (int64_t)1 << 31;
constexpr int kVoxelLog2Min = 6, kVoxelLog2Max = 32;   // a table has 64 .. 2^32 slots

// The table of a cloud of M voxels before a call of n items (log2cap: its slots now, 0: no table yet).
// Every item may bring a new key, and the table stays at most half full: M + n <= cap / 2 keeps it, else
// it grows to the power of two >= 2 (M + n), at least 64 slots and at most 2^32.  -> log2 of the slots
MC_CORE_HD int voxel_table_log2(int64_t M, int64_t n, int log2cap) {
  const int64_t need = M + n;
  if (log2cap > 0 && need <= (((int64_t)1 << log2cap) >> 1)) return log2cap;
  int l = kVoxelLog2Min;
  while (l < kVoxelLog2Max && ((int64_t)1 << l) < 2 * need) ++l;
  return l > log2cap ? l : log2cap;
}

// A voxel record offered to a merge: n points of voxel k arriving together with sums S[3] and SI.
// What n points can sum to: 0 <= Q <= 2^32 and |QI| <= 2^32 each.
MC_CORE_HD bool voxel_record_ok(const int32_t k[3], int64_t n, const int64_t S[3], int64_t SI) {
  if (n < 1 || n >= kVoxelPointsEnd) return false;
  const int64_t top = n << 32;   // < 2^63
  for (int c = 0; c < 3; ++c)
    if (k[c] < kVoxelKeyMin || k[c] >= kVoxelKeyEnd || S[c] < 0 || S[c] > top) return false;
  return SI >= -top && SI <= top;
}

// ---- shrinking a live cloud (voxel.hpp "taking voxels and points out") --------------------------------
// The table of a cloud that a removal leaves with M_keep voxels (log2cap: its slots now, 0: no table).  It stays
// unless the survivors fill less than an eighth of it; then it shrinks to the power of two >= 4 M_keep, at least
// 64 slots: a quarter full at most, so the next inserts find the room a build would have left them.  Never
// larger than it was.  -> log2 of the slots
MC_CORE_HD int voxel_table_shrink_log2(int64_t M_keep, int log2cap) {
  if (log2cap <= 0 || M_keep >= (((int64_t)1 << log2cap) >> 3)) return log2cap;
  int l = kVoxelLog2Min;
  while (l < log2cap && ((int64_t)1 << l) < 4 * M_keep) ++l;
  return l;
}

// What a subtraction leaves of a voxel's record: n points with sums S[3] and SI.  n = 0 with every sum 0 is a
// voxel that leaves; n >= 1 is held to what n points can sum to (voxel_record_ok's rule); anything else (n < 0,
// n = 0 with a sum left over, a sum outside its range) is no set of points.
MC_CORE_HD bool voxel_remainder_ok(int64_t n, const int64_t S[3], int64_t SI) {
  if (n < 0 || n >= kVoxelPointsEnd) return false;
  if (n == 0) return S[0] == 0 && S[1] == 0 && S[2] == 0 && SI == 0;
  const int64_t top = n << 32;   // < 2^63
  for (int c = 0; c < 3; ++c)
    if (S[c] < 0 || S[c] > top) return false;
  return SI >= -top && SI <= top;
}

// one voxel: out = cx, cy, cz, intensity (n >= 1)
MC_CORE_HD void voxel_finalise(const int32_t k[3], const int64_t S[3], int64_t SI, int64_t n, double h,
                                const double o[3], double out[4]) {
  MC_CORE_NO_CONTRACT
  const double dn = (double)n;
  for (int c = 0; c < 3; ++c) {
    const double m = (double)S[c] / dn;
    const double s = m * kVoxelFracInv;
    const double w = (double)k[c] + s;
    const double t = w * h;
    out[c] = o[c] + t;
  }
  const double mi = (double)SI / dn;
  out[3] = mi * kVoxelIntInv;
}

}  // namespace mc
