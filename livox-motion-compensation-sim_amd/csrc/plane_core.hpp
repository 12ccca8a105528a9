// plane_core.hpp — the scalar core of the voxel cloud's plane segmentation (plane.hpp), on plain values so the
// same text compiles for the device and for the host (tests/host/plane_host.cpp includes it; built with
// g++ -ffp-contract=off).  A core header (DESIGN.md "Core headers"); needs no stand-in.  No HIP include.
//
// RANSAC over the centroids c_v of the candidate voxels ids[0 .. n) (ascending voxel ids), defined op for op
// (include/mcdeskew.h "plane segmentation of the voxel cloud"):
//   sampler     r_j = mix(seed + GOLDEN (3k + j + 1)), j = 0, 1, 2 (splitmix64's finaliser, uint64 wrapping)
//               a = mulhi(r0, n)   b = mulhi(r1, n - 1), b++ if b >= a
//               c = mulhi(r2, n - 2), c++ if c >= min(a, b), then c++ if c >= max(a, b)
//   hypothesis  e1 = p1 - p0   e2 = p2 - p0   n = e1 x e2   l2 = (nx nx + ny ny) + nz nz
//               d = -((nx p0x + ny p0y) + nz p0z)   tau = (t t) l2
//               valid iff l2 > 0 and l2, d, tau finite; an invalid one is stored with tau = -1 and n = d = 0
//   score       s = ((nx cx + ny cy) + nz cz) + d; an inlier iff s s <= tau; the score is the number of inliers
//   winner      the highest score of at least 3, ties to the lowest k
//   model       l = sqrt(l2), n^ = n / l, d^ = -((n^x p0x + n^y p0y) + n^z p0z), negated as a whole when the
//               component of largest magnitude is negative (the lowest axis wins a tie)
//   refit       u = c_v - p0 and its six products per inlier (+0.0 otherwise), each of the nine summed by the
//               balanced adjacent-pair tree over the voxel ids padded to a power of two >= max(M, 256);
//               normals_covariance and normals_eigenvector of normals_core.hpp; q = p0 + m;
//               d^ = -((n^x qx + n^y qy) + n^z qz); an inlier iff fabs(((n^x cx + n^y cy) + n^z cz) + d^) <= t
// Every line of floating-point arithmetic is ONE IEEE float64 operation, never contracted.
#pragma once
#include <math.h>
#include <stdint.h>

#include "normals_core.hpp"

namespace mc {

constexpr uint64_t kPlaneGolden = 0x9E3779B97F4A7C15ull;
constexpr int32_t kPlaneMaxIterations = 1 << 20;
constexpr int64_t kPlaneLeavesMin = 256;   // the tree's leaves: a power of two >= max(M, 256)
constexpr int kPlaneSums = 9;              // s[3], P[6]
constexpr int kPlaneHyp = 8;               // float64 words per hypothesis record

// a hypothesis as the sample phase stores it (64 bytes); valid iff tau >= 0
struct PlaneHyp {
  double n[3];
  double d;
  double tau;
  double p0[3];
};

MC_CORE_HD uint64_t plane_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the high 64 bits of a * b, from 32-bit halves (the same text on both sides)
MC_CORE_HD uint64_t plane_mulhi(uint64_t a, uint64_t b) {
  const uint64_t al = a & 0xFFFFFFFFu, ah = a >> 32, bl = b & 0xFFFFFFFFu, bh = b >> 32;
  const uint64_t ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
  const uint64_t mid = (ll >> 32) + (lh & 0xFFFFFFFFu) + (hl & 0xFFFFFFFFu);
  return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// the three places in ids of hypothesis k (n >= 3 candidates): distinct by construction
MC_CORE_HD void plane_sample(uint64_t seed, uint32_t k, uint64_t n, uint64_t at[3]) {
  const uint64_t base = 3ull * k;
  const uint64_t r0 = plane_mix(seed + kPlaneGolden * (base + 1));
  const uint64_t r1 = plane_mix(seed + kPlaneGolden * (base + 2));
  const uint64_t r2 = plane_mix(seed + kPlaneGolden * (base + 3));
  const uint64_t a = plane_mulhi(r0, n);
  uint64_t b = plane_mulhi(r1, n - 1);
  if (b >= a) ++b;
  uint64_t c = plane_mulhi(r2, n - 2);
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
  if (c >= lo) ++c;
  if (c >= hi) ++c;
  at[0] = a;
  at[1] = b;
  at[2] = c;
}

// the plane through p0, p1, p2, unnormalised; tt = t * t
MC_CORE_HD PlaneHyp plane_hypothesis(const double p0[3], const double p1[3], const double p2[3], double tt) {
  MC_CORE_NO_CONTRACT
  const double e1x = p1[0] - p0[0];
  const double e1y = p1[1] - p0[1];
  const double e1z = p1[2] - p0[2];
  const double e2x = p2[0] - p0[0];
  const double e2y = p2[1] - p0[1];
  const double e2z = p2[2] - p0[2];
  const double a1 = e1y * e2z;
  const double a2 = e1z * e2y;
  const double b1 = e1z * e2x;
  const double b2 = e1x * e2z;
  const double c1 = e1x * e2y;
  const double c2 = e1y * e2x;
  const double nx = a1 - a2;
  const double ny = b1 - b2;
  const double nz = c1 - c2;
  const double xx = nx * nx;
  const double yy = ny * ny;
  const double zz = nz * nz;
  const double xy = xx + yy;
  const double l2 = xy + zz;
  const double px = nx * p0[0];
  const double py = ny * p0[1];
  const double pz = nz * p0[2];
  const double pxy = px + py;
  const double pd = pxy + pz;
  const double d = -pd;
  const double tau = tt * l2;
  PlaneHyp h;
  const bool valid = l2 > 0.0 && voxel_finite(l2) && voxel_finite(d) && voxel_finite(tau);
  h.n[0] = valid ? nx : 0.0;
  h.n[1] = valid ? ny : 0.0;
  h.n[2] = valid ? nz : 0.0;
  h.d = valid ? d : 0.0;
  h.tau = valid ? tau : -1.0;
  h.p0[0] = p0[0];
  h.p0[1] = p0[1];
  h.p0[2] = p0[2];
  return h;
}

// s of a centroid under (nx, ny, nz, d)
MC_CORE_HD double plane_offset(double nx, double ny, double nz, double d, double cx, double cy, double cz) {
  MC_CORE_NO_CONTRACT
  const double ax = nx * cx;
  const double ay = ny * cy;
  const double az = nz * cz;
  const double axy = ax + ay;
  const double a = axy + az;
  return a + d;
}

// the score's test (an invalid hypothesis has tau = -1: never)
MC_CORE_HD bool plane_inlier(double nx, double ny, double nz, double d, double tau, double cx, double cy, double cz) {
  MC_CORE_NO_CONTRACT
  const double s = plane_offset(nx, ny, nz, d, cx, cy, cz);
  const double ss = s * s;
  return ss <= tau;
}

// the refined model's test
MC_CORE_HD bool plane_within(double nx, double ny, double nz, double d, double t, double cx, double cy, double cz) {
  return fabs(plane_offset(nx, ny, nz, d, cx, cy, cz)) <= t;
}

// a voxel's nine leaves: u = c - p0 and its products for an inlier, +0.0 otherwise
MC_CORE_HD void plane_leaf(bool inlier, const double c[3], const double p0[3], double leaf[kPlaneSums]) {
  MC_CORE_NO_CONTRACT
  const double ux = c[0] - p0[0];
  const double uy = c[1] - p0[1];
  const double uz = c[2] - p0[2];
  const double xx = ux * ux;
  const double xy = ux * uy;
  const double xz = ux * uz;
  const double yy = uy * uy;
  const double yz = uy * uz;
  const double zz = uz * uz;
  leaf[0] = inlier ? ux : 0.0;
  leaf[1] = inlier ? uy : 0.0;
  leaf[2] = inlier ? uz : 0.0;
  leaf[3] = inlier ? xx : 0.0;
  leaf[4] = inlier ? xy : 0.0;
  leaf[5] = inlier ? xz : 0.0;
  leaf[6] = inlier ? yy : 0.0;
  leaf[7] = inlier ? yz : 0.0;
  leaf[8] = inlier ? zz : 0.0;
}

// the tree's leaves for M voxels
MC_CORE_HD int64_t plane_leaves(int64_t M) {
  int64_t L = kPlaneLeavesMin;
  while (L < M) L <<= 1;
  return L;
}

// the balanced adjacent-pair tree over a[0 .. count) at stride `stride`, count a power of two, in place -> a[0]
MC_CORE_HD double plane_tree(double* a, int64_t count, int64_t stride) {
  MC_CORE_NO_CONTRACT
  for (int64_t n = count; n > 1; n >>= 1)
    for (int64_t i = 0; i < n / 2; ++i) a[i * stride] = a[2 * i * stride] + a[(2 * i + 1) * stride];
  return a[0];
}

// the winner of score[0 .. K): the highest score of at least 3, ties to the lowest k; -1: none
MC_CORE_HD int32_t plane_pick(const uint32_t* score, int32_t K) {
  int32_t best = -1;
  uint32_t top = 2;
  for (int32_t k = 0; k < K; ++k)
    if (score[k] > top) {
      top = score[k];
      best = k;
    }
  return best;
}

// negate (n, d) when the component of n of largest magnitude is negative (the lowest axis wins a tie)
MC_CORE_HD void plane_sign(double model[4]) {
  double big = model[0];
  if (fabs(model[1]) > fabs(big)) big = model[1];
  if (fabs(model[2]) > fabs(big)) big = model[2];
  if (big < 0.0)
    for (int c = 0; c < 4; ++c) model[c] = -model[c];
}

// d^ of a unit normal through the point q
MC_CORE_HD double plane_d(const double nrm[3], const double q[3]) {
  MC_CORE_NO_CONTRACT
  const double px = nrm[0] * q[0];
  const double py = nrm[1] * q[1];
  const double pz = nrm[2] * q[2];
  const double pxy = px + py;
  const double pd = pxy + pz;
  return -pd;
}

// the model of the winning hypothesis itself (refine = false)
MC_CORE_HD void plane_model(const PlaneHyp& h, double model[4]) {
  MC_CORE_NO_CONTRACT
  const double xx = h.n[0] * h.n[0];
  const double yy = h.n[1] * h.n[1];
  const double zz = h.n[2] * h.n[2];
  const double xy = xx + yy;
  const double l2 = xy + zz;
  const double l = sqrt(l2);
  model[0] = h.n[0] / l;
  model[1] = h.n[1] / l;
  model[2] = h.n[2] / l;
  model[3] = plane_d(model, h.p0);
  plane_sign(model);
}

// the refit: sums = s[3], P[6] of the n_in >= 3 inliers about p0 -> model, cov = xx, xy, xz, yy, yz, zz
MC_CORE_HD void plane_refit(const double sums[kPlaneSums], int32_t n_in, const double p0[3], double model[4], double cov[6]) {
  MC_CORE_NO_CONTRACT
  NormalsMoments m;
  for (int c = 0; c < 3; ++c) m.s[c] = sums[c];
  for (int c = 0; c < 6; ++c) m.P[c] = sums[3 + c];
  normals_covariance(m, n_in, cov);
  normals_eigenvector(cov, model);
  const double dn = (double)n_in;
  double q[3];
  for (int c = 0; c < 3; ++c) {
    const double mc = m.s[c] / dn;
    q[c] = p0[c] + mc;
  }
  // the sign first: d^ of the signed normal is the negation of the other's, bit for bit
  model[3] = 0.0;
  plane_sign(model);
  model[3] = plane_d(model, q);
}

}  // namespace mc
