// las_core.hpp — the per-record cores of the LAS 1.2 codec (las.hpp): las_encode_rec, las_decode_rec,
// las_time_ns.  A core header (DESIGN.md "Core headers"): the device compiles this text and so does
// tests/host/las_host.cpp.  Needs no stand-in.  No HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

struct LasRec {
  int32_t X[3];
  uint32_t intensity;
  double gps;
  int bad;   // 1: refused (a coordinate not finite or outside int32 after scaling, an intensity NaN or outside 0..65535)
};

// X = int32(rint((v - off) / scale)): subtract, IEEE divide, round half to even (numpy's np.round)
MC_CORE_DEV int las_fix(double v, double off, double scale, int32_t* X) {
  const double q = rint((v - off) / scale);
  const bool ok = q >= -2147483648.0 && q <= 2147483647.0;   // false for NaN
  *X = ok ? (int32_t)q : 0;
  return ok ? 0 : 1;
}

// c = x, y, z, intensity source, time source; intensity = trunc(c[3] * imul) as u16, gps = c[4] * tmul
// (tmul == 0: 0.0 whatever c[4] holds)
MC_CORE_DEV LasRec las_encode_rec(const double c[5], const double scale[3], const double off[3],
                                                 double imul, double tmul) {
  LasRec r;
  r.bad = 0;
  MC_CORE_UNROLL
  for (int k = 0; k < 3; ++k) r.bad |= las_fix(c[k], off[k], scale[k], &r.X[k]);
  const double t = c[3] * imul;
  const bool ok = t > -1.0 && t < 65536.0;   // truncation toward zero lands in 0..65535; false for NaN
  r.intensity = ok ? (uint32_t)(int32_t)t : 0u;
  r.bad |= ok ? 0 : 1;
  r.gps = tmul != 0.0 ? c[4] * tmul : 0.0;
  return r;
}

// x = X * scale + offset: the product rounded, then the sum rounded — never one fused multiply-add
// (hipcc contracts a * b + c by default, which changes the last bit of about a quarter of the values
// at scale 0.001 / offset 500000)
MC_CORE_DEV double las_unscale(int32_t X, double scale, double off) {
  MC_CORE_NO_CONTRACT
  const double p = (double)X * scale;
  return p + off;
}

MC_CORE_DEV uint32_t las_le32(const uint8_t* r) {
  return (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
}

// one record of format fmt (0..3) at r -> x, y, z, intensity, gps_time (0.0 for formats 0 and 2)
MC_CORE_DEV void las_decode_rec(const uint8_t* r, int fmt, const double scale[3], const double off[3],
                                               double v[5]) {
  MC_CORE_UNROLL
  for (int k = 0; k < 3; ++k) v[k] = las_unscale((int32_t)las_le32(r + 4 * k), scale[k], off[k]);
  v[3] = (double)((uint32_t)r[12] | ((uint32_t)r[13] << 8));
  v[4] = 0.0;
  if (fmt & 1) {
    const uint64_t b = (uint64_t)las_le32(r + 20) | ((uint64_t)las_le32(r + 24) << 32);
    v[4] = __builtin_bit_cast(double, b);
  }
}

// int64(rint(gps * 1e9)); false when that is NaN or outside int64
MC_CORE_DEV bool las_time_ns(double gps, int64_t* out) {
  const double t = rint(gps * 1e9);
  if (!(t >= -9223372036854775808.0 && t < 9223372036854775808.0)) return false;
  *out = (int64_t)t;
  return true;
}

}  // namespace mc
