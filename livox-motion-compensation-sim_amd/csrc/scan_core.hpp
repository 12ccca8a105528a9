// scan_core.hpp — the visibility decision of the scene scanner (scan.hpp): ScanParams, make_scan_params,
// scan_rotate, scan_visible with its fast tier and the reference's exact tier.  A core header (DESIGN.md "Core
// headers"): the device compiles this text and so does tests/host/scan_host.cpp, which counts the exact tier's
// atan2 / asin calls.  Needs no stand-in.  No HIP include.
#pragma once
#include <cmath>
#include <math.h>
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

struct ScanParams {
  double range_min, range_max_sq, half_fov_h, half_fov_v;
  int64_t cap;         // points_per_frame
  double tan_h, sin_v2;        // tan / sin^2 of the half FOVs: decisions away from the edges
  double rmin2_lo, rmin2_hi;   // range_min^2 (1 -+ 1e-12)
  int fast;                    // both half FOVs in [0, 89) degrees
};

inline ScanParams make_scan_params(const double par[4], int64_t cap) {
  ScanParams sp;
  sp.range_min = par[0]; sp.range_max_sq = par[1]; sp.half_fov_h = par[2]; sp.half_fov_v = par[3];
  sp.cap = cap;
  const double d2r = 3.141592653589793 / 180.0;
  sp.fast = par[2] >= 0.0 && par[2] < 89.0 && par[3] >= 0.0 && par[3] < 89.0;
  sp.tan_h = sp.fast ? std::tan(par[2] * d2r) : 0.0;
  const double sv = sp.fast ? std::sin(par[3] * d2r) : 0.0;
  sp.sin_v2 = sv * sv;
  // a non-positive range_min passes every point (sqrt(d2) >= 0)
  sp.rmin2_lo = par[0] > 0.0 ? par[0] * par[0] * (1.0 - 1e-12) : -1.0;
  sp.rmin2_hi = par[0] > 0.0 ? par[0] * par[0] * (1.0 + 1e-12) : -1.0;
  return sp;
}

// R^T d (LMC:728: (R.T @ d.T).T) the way numpy's matmul accumulates it: per output an ascending
// FMA chain over k, fma(A[i][2], d2, fma(A[i][1], d1, A[i][0] * d0)) with A = R^T (numpy's dgemm on
// the reference's box, tools/fma_order.py).  With the pose's R from rot.cpp the sensor-frame
// coordinates equal the reference's bit for bit.
MC_CORE_DEV void scan_rotate(const double* __restrict__ P, double dx, double dy, double dz, double& lx,
                                            double& ly, double& lz) {
  MC_CORE_NO_CONTRACT
  lx = __builtin_fma(P[6], dz, __builtin_fma(P[3], dy, P[0] * dx));
  ly = __builtin_fma(P[7], dz, __builtin_fma(P[4], dy, P[1] * dx));
  lz = __builtin_fma(P[8], dz, __builtin_fma(P[5], dy, P[2] * dx));
}

// the reference's degree comparisons (LMC:735-744), for points near an FOV edge only: kept out of
// line so the rarely taken transcendental code does not inflate the register budget of the loop
MC_CORE_DEV_NOINLINE bool scan_fov_exact(double lx, double ly, double s, int az_in, int el_in, double half_h,
                                            double half_v) {
  if (az_in < 0 && !(fabs(atan2(ly, lx) * 180.0 / 3.141592653589793) <= half_h)) return false;
  if (el_in < 0 && !(fabs(asin(s) * 180.0 / 3.141592653589793) <= half_v)) return false;
  return true;
}

// LMC:713-745 for one scene point (ex, ey, ez); returns visibility and the sensor-frame coordinates
MC_CORE_DEV bool scan_visible(const double* __restrict__ P, double ex, double ey, double ez,
                                             const ScanParams& sp, double& lx, double& ly, double& lz) {
  MC_CORE_NO_CONTRACT
  const double dx = ex - P[9], dy = ey - P[10], dz = ez - P[11];
  const double d2 = dx * dx + dy * dy + dz * dz;              // np.sum(.., axis=1) order
  if (!(d2 <= sp.range_max_sq)) return false;                 // LMC:718
  scan_rotate(P, dx, dy, dz, lx, ly, lz);                      // R^T (p - t), LMC:727-728
  // Away from the edges the tests of LMC:732-745 are decided without sqrt / division / atan2 /
  // asin: r >= range_min by d2 against range_min^2, |az| <= h by |ly| <= tan(h) lx (lx > 0),
  // |el| <= v by lz^2 <= sin(v)^2 d2 (both FOVs below 90 degrees, where atan2 / asin are
  // monotonic).  Within a relative 1e-9 of any edge the reference's own expressions decide.
  int r_in = -1, az_in = -1, el_in = -1;
  if (sp.fast) {
    r_in = d2 > sp.rmin2_hi ? 1 : (d2 < sp.rmin2_lo ? 0 : -1);
    const double m = 1e-9 * (fabs(lx) + fabs(ly) + fabs(lz));
    const double a = fabs(ly) - sp.tan_h * lx;
    if (lx > m) az_in = a < -m ? 1 : (a > m ? 0 : -1);
    else if (lx < -m) az_in = 0;
    if (d2 > 1e-10) {
      const double e = lz * lz - sp.sin_v2 * d2;
      const double me = 1e-9 * d2;
      el_in = e < -me ? 1 : (e > me ? 0 : -1);
    }
    if (r_in == 0 || az_in == 0 || el_in == 0) return false;
    if (r_in == 1 && az_in == 1 && el_in == 1) return true;
  }
  const double r = sqrt(d2);                                   // LMC:732
  if (!(r >= sp.range_min)) return false;                      // LMC:745
  double s = lz / fmax(r, 1e-6);                               // LMC:738-739
  s = fmin(fmax(s, -1.0), 1.0);
  return scan_fov_exact(lx, ly, s, az_in, el_in, sp.half_fov_h, sp.half_fov_v);
}

}  // namespace mc
