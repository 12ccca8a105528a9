// relfold.hpp — the algebra of the relative (sensor-frame) SLERP deskew, on plain double arrays so
// the same text compiles for the device (kernels.hpp, relative.hpp) and for the host (tests/test_relative_cpu.py
// builds it with g++ -ffp-contract=off).  No HIP include.
//
// The SLERP record is linear in what the deskew kernel evaluates,
//   q(alpha) = cos(alpha Theta) q0 + alpha sinc(alpha Theta) v,   pos(alpha) = p0 + alpha dp,
// so the inverse of a reference pose (q_ref, pos_ref) folds into the record once:
//   q0' = conj(q_ref) (x) q0,  v' = conj(q_ref) (x) v,  p0' = R_ref^T (p0 - pos_ref),  dp' = R_ref^T dp
// and slerp_core on the primed record yields p' = R_ref^T (R(q(t)) p + pos(t) - pos_ref) directly
// (Theta, t0, inv_dt and tf are unchanged).  Quaternions are (x, y, z, w), as PoseSeg holds them.
#pragma once

#include "core_fn.hpp"

namespace mc {

// o = conj(r) (x) q (Hamilton product): R(o) = R(r)^T R(q)
MC_CORE_HD void quat_conj_mul(const double r[4], const double q[4], double o[4]) {
  const double ax = -r[0], ay = -r[1], az = -r[2], aw = r[3];
  o[0] = aw * q[0] + ax * q[3] + ay * q[2] - az * q[1];
  o[1] = aw * q[1] - ax * q[2] + ay * q[3] + az * q[0];
  o[2] = aw * q[2] + ax * q[1] - ay * q[0] + az * q[3];
  o[3] = aw * q[3] - ax * q[0] - ay * q[1] - az * q[2];
}

// o = R(r)^T v: v rotated by conj(r), v + 2 (w t + u x t) with u = -r.xyz, t = u x v (slerp_core's form)
MC_CORE_HD void quat_rot_inv(const double r[4], const double v[3], double o[3]) {
  const double ux = -r[0], uy = -r[1], uz = -r[2], w = r[3];
  const double tx = uy * v[2] - uz * v[1];
  const double ty = uz * v[0] - ux * v[2];
  const double tz = ux * v[1] - uy * v[0];
  o[0] = v[0] + 2.0 * (w * tx + (uy * tz - uz * ty));
  o[1] = v[1] + 2.0 * (w * ty + (uz * tx - ux * tz));
  o[2] = v[2] + 2.0 * (w * tz + (ux * ty - uy * tx));
}

// the record (q0, v, p0, dp) of one pose segment, in place, into the frame of (q_ref, pos_ref); the
// cancellation p0 - pos_ref happens here, once per record, in float64
MC_CORE_HD void rel_fold(const double q_ref[4], const double pos_ref[3], double q0[4], double v[4], double p0[3],
                            double dp[3]) {
  const double a[4] = {q0[0], q0[1], q0[2], q0[3]}, b[4] = {v[0], v[1], v[2], v[3]};
  const double d[3] = {p0[0] - pos_ref[0], p0[1] - pos_ref[1], p0[2] - pos_ref[2]};
  const double e[3] = {dp[0], dp[1], dp[2]};
  quat_conj_mul(q_ref, a, q0);
  quat_conj_mul(q_ref, b, v);
  quat_rot_inv(q_ref, d, p0);
  quat_rot_inv(q_ref, e, dp);
}

}  // namespace mc
