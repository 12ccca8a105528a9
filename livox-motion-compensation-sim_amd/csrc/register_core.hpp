// register_core.hpp — the scalar core of the point-to-plane registration of a source against the voxel cloud
// (register.hpp), on plain values so the same text compiles for the device and for the host
// (tests/host/register_host.cpp and register_frames_host.cpp include it; built with g++ -ffp-contract=off).  A core
// header (DESIGN.md "Core headers"); needs no stand-in.  No HIP include.
//
// Defined op for op (include/mcdeskew.h "registration against the voxel cloud"); p a source point, (R, t) the pose:
//   move      q = R p + t, each component ((R0 x + R1 y) + R2 z) + t
//   cell      voxel_quantise's k of q with the build's h and origin; a q it refuses has no pair
//   nearest   the window walk of normals_core.hpp around that cell with ci = q, W = ceil(max_distance / h) and
//             r2 = max_distance^2: the smallest d2 <= r2, ties to the lower window index (the lower cell key); the
//             walk leaves out cells that cannot hold it (RegSkip), which changes no output
//   pair      the nearest voxel v when its normal was estimated from three neighbours or more
//   leaves    d = q - c_v   r = (nx dx + ny dy) + nz dz   a = q x n, each component (u*v) - (w*x)   J = (a, n)
//             the 21 products J_i J_j (i <= j, row-major), the 6 products J_i r, and r r; +0.0 without a pair
//   sums      each of the 28 by the balanced adjacent-pair tree of plane_core.hpp over the source point index
//   step      A x = -b by Cholesky (A = L L^T row by row, inner sums in ascending index, then L y = -b and
//             L^T x = y); a pivot that is not finite or not > 0: singular; x = (w, v)
//   update    the unit quaternion (1, w / 2) / |(1, w / 2)| as a rotation dR (one sqrt, no trigonometry);
//             R <- dR R, t <- dR t + v
//   stop      converged when w.w <= tol_rotation^2 and v.v <= tol_translation^2
// Every line of floating-point arithmetic is ONE IEEE float64 operation, never contracted.
#pragma once
#include <math.h>
#include <stdint.h>

#include "normals_core.hpp"
#include "plane_core.hpp"

namespace mc {

constexpr int kRegSums = 28;          // J J^T's upper triangle (21), J r (6), r r (1)
constexpr int kRegHistory = 8;        // pairs, sum r r, w[3], v[3] per iteration
constexpr int64_t kRegMinPairs = 6;
constexpr int32_t kRegMaxIterations = 1 << 16;
enum { kRegConverged = 0, kRegMaxIter = 1, kRegTooFewPairs = 2, kRegSingular = 3, kRegGoOn = -1 };

struct RegPose {
  double R[9];   // row-major
  double t[3];
};

MC_CORE_HD void register_move(const RegPose& T, const double p[3], double q[3]) {
  MC_CORE_NO_CONTRACT
  for (int c = 0; c < 3; ++c) {
    const double ax = T.R[3 * c] * p[0];
    const double ay = T.R[3 * c + 1] * p[1];
    const double az = T.R[3 * c + 2] * p[2];
    const double axy = ax + ay;
    const double a = axy + az;
    q[c] = a + T.t[c];
  }
}

// What the nearest-centroid walk may leave out (the definition's point 3): a plane, row or cell of the window whose
// box is farther from q than `bound`, the smaller of r2 and the smallest d2 known, cannot hold the winner or a tie
// with it.  The distance to the box is taken low: every axis gap is shortened by 2^-48 of the coordinates' size (a
// centroid may lie an ulp or two outside its cell's computed faces) and the sum by 2^-30, far more than the rounding
// of d2 itself, so a cell is left out only when every centroid it could hold has d2 > bound as the walk computes it.
struct RegSkip {
  const double* q;
  const double* o;
  double h;
  const double* bound;
  // the squared gap, taken low, between q and cell index k on one axis
  MC_CORE_HD double gap2(int a, int32_t k) const {
    const double lo = o[a] + (double)k * h;
    const double hi = o[a] + (double)(k + 1) * h;
    const double slack = 3.552713678800501e-15 * ((fabs(lo) + fabs(hi)) + fabs(q[a]));   // 2^-48
    double gap = lo - q[a] > q[a] - hi ? lo - q[a] : q[a] - hi;
    gap = gap - slack;
    return gap > 0.0 ? gap * gap : 0.0;
  }
  MC_CORE_HD bool far(double sum) const { return sum * 0.999999999 > *bound; }
  MC_CORE_HD bool plane(int32_t kx) const { return far(gap2(0, kx)); }
  MC_CORE_HD bool row(int32_t kx, int32_t ky) const { return far(gap2(0, kx) + gap2(1, ky)); }
  MC_CORE_HD bool cell(const int32_t* k) const { return far((gap2(0, k[0]) + gap2(1, k[1])) + gap2(2, k[2])); }
};

// the voxel whose centroid is nearest to q within the window (w.R cells, w.r2; w.max_nn unused): -> found;
// *id = -1 and *d2 = inf without one.  Cells that cannot win are not probed (RegSkip); q's own cell is probed first
// for a bound, and then takes its turn in the walk like any other.
MC_CORE_HD bool register_nearest(const NormalsGrid& g, double h, const double o[3], const NormalsQuery& w, const double q[3],
                                 int32_t* id, double* d2) {
  MC_CORE_NO_CONTRACT
  int32_t best = -1, best_ix = 0;
  double best_d2 = (double)INFINITY;
  const VoxelPoint cell = voxel_quantise(q, 0.0, h, o);
  if (!cell.bad) {
    double bound = w.r2;
    auto take = [&](int32_t ix, uint32_t v, const double*, double dd) {
      if (best < 0 || normals_before(dd, ix, best_d2, best_ix)) {
        best = (int32_t)v;
        best_ix = ix;
        best_d2 = dd;
        if (dd < bound) bound = dd;
      }
    };
    uint32_t v;
    if (normals_find(g, voxel_pack(cell.k), &v)) {
      const double* c = g.cent + (int64_t)kNormalsCent * v;
      const double ux = c[0] - q[0];
      const double uy = c[1] - q[1];
      const double uz = c[2] - q[2];
      const double xx = ux * ux;
      const double yy = uy * uy;
      const double zz = uz * uz;
      const double xy = xx + yy;
      const double own = xy + zz;
      if (own < bound) bound = own;
    }
    const RegSkip skip = {q, o, h, &bound};
    normals_neighbours_v(g, cell.k, q, w, take, 0, skip);
  }
  *id = best;
  *d2 = best_d2;
  return best >= 0;
}

// a source point's 28 leaves: q against the centroid c and the normal n of its pair; +0.0 without one
MC_CORE_HD void register_leaf(bool pair, const double q[3], const double c[3], const double n[3], double leaf[kRegSums]) {
  MC_CORE_NO_CONTRACT
  const double dx = q[0] - c[0];
  const double dy = q[1] - c[1];
  const double dz = q[2] - c[2];
  const double rx = n[0] * dx;
  const double ry = n[1] * dy;
  const double rz = n[2] * dz;
  const double rxy = rx + ry;
  const double r = rxy + rz;
  const double a1 = q[1] * n[2];
  const double a2 = q[2] * n[1];
  const double b1 = q[2] * n[0];
  const double b2 = q[0] * n[2];
  const double c1 = q[0] * n[1];
  const double c2 = q[1] * n[0];
  double J[6];
  J[0] = a1 - a2;
  J[1] = b1 - b2;
  J[2] = c1 - c2;
  J[3] = n[0];
  J[4] = n[1];
  J[5] = n[2];
  int at = 0;
  MC_CORE_UNROLL
  for (int i = 0; i < 6; ++i) {
    MC_CORE_UNROLL
    for (int j = i; j < 6; ++j) {
      const double jj = J[i] * J[j];
      leaf[at++] = pair ? jj : 0.0;
    }
  }
  MC_CORE_UNROLL
  for (int i = 0; i < 6; ++i) {
    const double jr = J[i] * r;
    leaf[21 + i] = pair ? jr : 0.0;
  }
  const double rr = r * r;
  leaf[27] = pair ? rr : 0.0;
}

// A x = -b of the 28 sums by Cholesky: -> false when a pivot is not finite or not > 0 (x is then untouched)
MC_CORE_HD bool register_solve(const double s[kRegSums], double x[6]) {
  MC_CORE_NO_CONTRACT
  double A[6][6], L[6][6] = {}, y[6] = {}, out[6] = {};
  int at = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      A[i][j] = s[at];
      A[j][i] = s[at++];
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double acc = A[i][j];
      for (int k = 0; k < j; ++k) {
        const double p = L[i][k] * L[j][k];
        acc = acc - p;
      }
      if (j == i) {
        if (!(voxel_finite(acc) && acc > 0.0)) return false;
        L[i][i] = sqrt(acc);
      } else {
        L[i][j] = acc / L[j][j];
      }
    }
  for (int i = 0; i < 6; ++i) {
    double acc = -s[21 + i];
    for (int k = 0; k < i; ++k) {
      const double p = L[i][k] * y[k];
      acc = acc - p;
    }
    y[i] = acc / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double acc = y[i];
    for (int k = i + 1; k < 6; ++k) {
      const double p = L[k][i] * out[k];
      acc = acc - p;
    }
    out[i] = acc / L[i][i];
  }
  for (int i = 0; i < 6; ++i) x[i] = out[i];
  return true;
}

// the rotation of the unit quaternion (1, w / 2) / |(1, w / 2)|, row-major
MC_CORE_HD void register_rotation(const double w[3], double D[9]) {
  MC_CORE_NO_CONTRACT
  const double hx = 0.5 * w[0];
  const double hy = 0.5 * w[1];
  const double hz = 0.5 * w[2];
  const double sx = hx * hx;
  const double sy = hy * hy;
  const double sz = hz * hz;
  const double sxy = sx + sy;
  const double s3 = sxy + sz;
  const double n2 = 1.0 + s3;
  const double n = sqrt(n2);
  const double qw = 1.0 / n;
  const double qx = hx / n;
  const double qy = hy / n;
  const double qz = hz / n;
  const double xx = qx * qx;
  const double yy = qy * qy;
  const double zz = qz * qz;
  const double xy = qx * qy;
  const double xz = qx * qz;
  const double yz = qy * qz;
  const double wx = qw * qx;
  const double wy = qw * qy;
  const double wz = qw * qz;
  const double d0 = yy + zz;
  const double d1 = xx + zz;
  const double d2 = xx + yy;
  const double e0 = 2.0 * d0;
  const double e1 = 2.0 * d1;
  const double e2 = 2.0 * d2;
  const double f01 = xy - wz;
  const double f02 = xz + wy;
  const double f10 = xy + wz;
  const double f12 = yz - wx;
  const double f20 = xz - wy;
  const double f21 = yz + wx;
  D[0] = 1.0 - e0;
  D[1] = 2.0 * f01;
  D[2] = 2.0 * f02;
  D[3] = 2.0 * f10;
  D[4] = 1.0 - e1;
  D[5] = 2.0 * f12;
  D[6] = 2.0 * f20;
  D[7] = 2.0 * f21;
  D[8] = 1.0 - e2;
}

// R <- dR R, t <- dR t + v for the step x = (w, v)
MC_CORE_HD void register_update(RegPose* T, const double x[6]) {
  MC_CORE_NO_CONTRACT
  double D[9];
  register_rotation(x, D);
  RegPose N;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      const double a0 = D[3 * r] * T->R[c];
      const double a1 = D[3 * r + 1] * T->R[3 + c];
      const double a2 = D[3 * r + 2] * T->R[6 + c];
      const double a01 = a0 + a1;
      N.R[3 * r + c] = a01 + a2;
    }
    const double b0 = D[3 * r] * T->t[0];
    const double b1 = D[3 * r + 1] * T->t[1];
    const double b2 = D[3 * r + 2] * T->t[2];
    const double b01 = b0 + b1;
    const double b = b01 + b2;
    N.t[r] = b + x[3 + r];
  }
  *T = N;
}

MC_CORE_HD bool register_small(const double x[6], double tol_rotation, double tol_translation) {
  MC_CORE_NO_CONTRACT
  const double w0 = x[0] * x[0];
  const double w1 = x[1] * x[1];
  const double w2 = x[2] * x[2];
  const double w01 = w0 + w1;
  const double ww = w01 + w2;
  const double v0 = x[3] * x[3];
  const double v1 = x[4] * x[4];
  const double v2 = x[5] * x[5];
  const double v01 = v0 + v1;
  const double vv = v01 + v2;
  const double tr = tol_rotation * tol_rotation;
  const double tt = tol_translation * tol_translation;
  return ww <= tr && vv <= tt;
}

// One iteration's end, from its 28 sums and pair count: the history row, the step and the pose after it.
// -> kRegGoOn, or the status the registration ends with here (the pose is the one before a failed step)
MC_CORE_HD int register_step(const double sums[kRegSums], int64_t pairs, double tol_rotation, double tol_translation,
                             RegPose* T, double row[kRegHistory]) {
  row[0] = (double)pairs;
  row[1] = sums[27];
  for (int i = 0; i < 6; ++i) row[2 + i] = 0.0;
  if (pairs < kRegMinPairs) return kRegTooFewPairs;
  double x[6];
  if (!register_solve(sums, x)) return kRegSingular;
  for (int i = 0; i < 6; ++i) row[2 + i] = x[i];
  register_update(T, x);
  return register_small(x, tol_rotation, tol_translation) ? kRegConverged : kRegGoOn;
}

// ---- the frames of a batch registered together (register.hpp k_rg_frames_*; mc_voxel_register_frames) -------------
// Frame f is a source of its own: its points indexed within the frame, its own tree over plane_leaves(n) leaves, its
// own pair count, step and stop; nothing couples the frames.  A frame that has ended is not touched again.
constexpr int kRegEmpty = 4;          // the status of a frame without points (after the four of a registration)
constexpr int kRegBlock = (int)kPlaneLeavesMin;   // leaves per workgroup of the first level and per node of every further one
constexpr int kRegTopMax = kRegBlock / 2;   // a frame's last level holds fewer than 256 partials per sum: <= 128

struct RegFrame {
  RegPose T;
  unsigned long long count;   // the pairs of the iteration under way (the step kernel adds, the solve takes and zeroes)
  int64_t pairs;              // of the last evaluated iteration
  int64_t n;                  // points
  int64_t blocks;             // first-level partials per sum: plane_leaves(n) / 256; 0 for an empty frame
  int64_t tree;               // where the frame's levels start in the tree scratch (words), back to back as tree_words
  int64_t top;                // where its last level starts
  int32_t top_n;              // partials per sum there: < 256
  int32_t status;             // kRegGoOn while live
  int32_t iterations;
  int32_t pad_;
};

// The block map: off[0 .. F] a prefix of the frames' block counts, b in [0, off[F]) -> the frame that owns block b,
// the last one starting at or before it (a frame without blocks starts where the next begins and owns none)
MC_CORE_HD int32_t register_block_frame(const int64_t* off, int32_t F, int64_t b) {
  int32_t lo = 0, hi = F - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Where a frame of `blocks` first-level partials keeps level `level` (1: the first) relative to its `tree`, and the
// partials per sum there; a level has a successor while it holds 256 or more
MC_CORE_HD int64_t register_level(int64_t blocks, int level, int64_t* cnt) {
  int64_t at = 0, n = blocks;
  for (int l = 1; l < level; ++l) {
    at += (int64_t)kRegSums * n;
    n /= kRegBlock;
  }
  *cnt = n;
  return at;
}

// the record of a frame of n points from the pose T whose levels start at word `tree`: -> the words they take
MC_CORE_HD int64_t register_frame_init(RegFrame* fr, const RegPose& T, int64_t n, int64_t tree) {
  fr->T = T;
  fr->count = 0;
  fr->pairs = 0;
  fr->n = n;
  fr->tree = tree;
  fr->iterations = 0;
  fr->pad_ = 0;
  if (n == 0) {
    fr->blocks = 0;
    fr->top = tree;
    fr->top_n = 0;
    fr->status = kRegEmpty;
    return 0;
  }
  fr->blocks = plane_leaves(n) / kRegBlock;
  int64_t cnt = fr->blocks, at = 0;
  while (cnt >= kRegBlock) {
    at += (int64_t)kRegSums * cnt;
    cnt /= kRegBlock;
  }
  fr->top = tree + at;
  fr->top_n = (int32_t)cnt;
  fr->status = kRegGoOn;
  return at + (int64_t)kRegSums * cnt;
}

// the last levels of one sum: top[0 .. cnt) (cnt a power of two below 256) by plane_tree's pairing, in place
MC_CORE_HD double register_tail(double* top, int64_t cnt) { return plane_tree(top, cnt, 1); }

// The end of a live frame's iteration from its 28 sums: register_step with the pairs counted, the history row
// rows[iterations], and the record for the next iteration (the counter zeroed).  max_iterations reached without
// another ending: kRegMaxIter.  -> the frame is still live
MC_CORE_HD bool register_frame_end(RegFrame* fr, const double sums[kRegSums], int32_t max_iterations, double tol_rotation,
                                   double tol_translation, double* rows) {
  const int64_t pairs = (int64_t)fr->count;
  int status = register_step(sums, pairs, tol_rotation, tol_translation, &fr->T, rows + (int64_t)kRegHistory * fr->iterations);
  fr->pairs = pairs;
  fr->count = 0;
  fr->iterations += 1;
  if (status == kRegGoOn && fr->iterations >= max_iterations) status = kRegMaxIter;
  fr->status = status;
  return status == kRegGoOn;
}

// what a pose argument must hold: finite entries and |R^T R - I| <= 1e-6 in every entry
MC_CORE_HD bool register_pose_ok(const RegPose& T) {
  for (int i = 0; i < 9; ++i) if (!voxel_finite(T.R[i])) return false;
  for (int i = 0; i < 3; ++i) if (!voxel_finite(T.t[i])) return false;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double g = (T.R[a] * T.R[b] + T.R[3 + a] * T.R[3 + b]) + T.R[6 + a] * T.R[6 + b];
      if (!(fabs(g - (a == b ? 1.0 : 0.0)) <= 1e-6)) return false;
    }
  return true;
}

}  // namespace mc
