// raymarch_core.hpp — the per-pair core of the ray-march scanner (raymarch.hpp): the conservative tube test,
// the reference's exact predicate, the hit key and its order.  A core header (DESIGN.md "Core headers"): the
// device compiles this text and so does tests/host/raymarch_host.cpp.  Needs no stand-in.  No HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mcray {

// (step << 32 | object), the distance's bits (non-negative doubles order as their bits), scene index
struct RayKey {
  uint64_t ko, dist, idx;
};
constexpr uint64_t kRayMiss = ~0ull;

MC_CORE_HD_INLINE bool ray_key_less(const RayKey& a, const RayKey& b) {
  if (a.ko != b.ko) return a.ko < b.ko;
  if (a.dist != b.dist) return a.dist < b.dist;
  return a.idx < b.idx;
}

struct Ray {
  double ox, oy, oz;   // sensor position
  double wx, wy, wz;   // world direction R @ direction
};

// the march of one call: steps[k] = np.arange(range_min, range_max, step)[k], uploaded from numpy
struct RayMarch {
  double range_min;    // steps[0]
  double step;         // 0.1: the step size and the hit radius (CSIM:1118, 1131)
  double s_lo, s_hi;   // along-ray coordinates a close point can have: the marched range +- 2 steps
  double tube2;        // (step (1 + 1e-5))^2
  int32_t K;           // number of steps
};

MC_CORE_HD_INLINE RayMarch make_ray_march(const double* steps, int32_t K, double step) {
  RayMarch m;
  m.K = K;
  m.step = step;
  m.range_min = K > 0 ? steps[0] : 0.0;
  m.s_lo = m.range_min - 2.0 * step;
  m.s_hi = (K > 0 ? steps[K - 1] : 0.0) + 2.0 * step;
  const double t = step * (1.0 + 1e-5);
  m.tube2 = t * t;
  return m;
}

// R @ d for one vector, numpy's one-row (matrix-vector) order for a 3x3:
// fma(a2, x2, fma(a0, x0, a1 * x1)).  Forms the world direction (CSIM:1105-1106) and the
// sensor-frame point (CSIM:1170-1171).
MC_CORE_HD_INLINE void ray_rotate(const double* A, double x, double y, double z, double& ox, double& oy, double& oz) {
  MC_CORE_NO_CONTRACT
  ox = __builtin_fma(A[2], z, __builtin_fma(A[0], x, A[1] * y));
  oy = __builtin_fma(A[5], z, __builtin_fma(A[3], x, A[4] * y));
  oz = __builtin_fma(A[8], z, __builtin_fma(A[6], x, A[7] * y));
}

// current_point = origin + direction * distance (CSIM:1122): a multiply, then an add
MC_CORE_HD_INLINE void ray_sample(const Ray& r, double d, double& cx, double& cy, double& cz) {
  MC_CORE_NO_CONTRACT
  const double mx = r.wx * d, my = r.wy * d, mz = r.wz * d;
  cx = r.ox + mx;
  cy = r.oy + my;
  cz = r.oz + mz;
}

// Conservative filter: false only for points that cannot be within `step` of any sample of the ray
// (ray_tube) up to along-ray coordinate s_max (ray_in_range).  Rounding here (contraction allowed) is ~1e-11 at 260 m, far inside the
// 1e-5 relative widening of the tube.
MC_CORE_HD_INLINE bool ray_tube(const Ray& r, const RayMarch& m, double px, double py, double pz, double& s) {
  const double vx = px - r.ox, vy = py - r.oy, vz = pz - r.oz;
  s = vx * r.wx + vy * r.wy + vz * r.wz;
  const double v2 = vx * vx + vy * vy + vz * vz;
  const double perp2 = v2 - s * s;
  return perp2 <= m.tube2;
}
// ... and, for the few points inside the tube, the along-ray range
MC_CORE_HD_INLINE bool ray_in_range(const RayMarch& m, double s_max, double s) { return s >= m.s_lo && s <= s_max; }

// The reference's predicate (CSIM:1122, 1130-1131) for a tube candidate at the steps around s: the
// first step with distance < step gives this point's key; `best` keeps the minimum.
MC_CORE_HD_NOINLINE void ray_exact(const Ray& r, const RayMarch& m, const double* steps, double px, double py,
                                   double pz, double s, uint32_t obj, uint64_t idx, RayKey& best) {
  MC_CORE_NO_CONTRACT
  double q = floor((s - m.range_min) / m.step);
  q = q < -4.0 ? -4.0 : (q > (double)m.K + 4.0 ? (double)m.K + 4.0 : q);
  const int32_t k0 = (int32_t)q;
  const int32_t ka = k0 - 2 < 0 ? 0 : k0 - 2;
  const int32_t kb = k0 + 3 > m.K - 1 ? m.K - 1 : k0 + 3;
  for (int32_t k = ka; k <= kb; ++k) {
    double cx, cy, cz;
    ray_sample(r, steps[k], cx, cy, cz);
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    const double sq = (dx * dx + dy * dy) + dz * dz;   // np.add.reduce over the 3 squares
    const double dist = sqrt(sq);
    if (dist < m.step) {
      RayKey key;
      key.ko = ((uint64_t)(uint32_t)k << 32) | obj;
      __builtin_memcpy(&key.dist, &dist, 8);
      key.idx = idx;
      if (ray_key_less(key, best)) best = key;
      return;   // this point's later steps have larger keys
    }
  }
}

// after a hit at step k nothing with s > steps[k] + 2 step can beat it (a point close at a step
// <= k has s < steps[k] + step)
MC_CORE_HD_INLINE double ray_s_max(const RayMarch& m, const double* steps, const RayKey& best) {
  return best.ko == kRayMiss ? m.s_hi : steps[best.ko >> 32] + 2.0 * m.step;
}

}  // namespace mcray
