// normals_core.hpp — the scalar core of the voxel cloud's surface normals (normals.hpp), on plain values so
// the same text compiles for the device and for the host (tests/host/normals_host.cpp includes it; built with
// g++ -ffp-contract=off).  A core header (DESIGN.md "Core headers"); needs no stand-in.  No HIP include.
//
// The estimate of one voxel i is a function of the voxel set alone (include/mcdeskew.h "surface normals"):
//   candidates  the occupied cells k_j with max_axis |k_j - k_i| <= R, i itself included, walked in the
//               order dkx, dky, dkz ascending = ascending packed key; a cell with an index outside
//               [kVoxelKeyMin, kVoxelKeyEnd) on any axis is skipped before it is packed
//   radius      u = c_j - c_i     d2 = (u.x*u.x + u.y*u.y) + u.z*u.z     a neighbour when d2 <= r2
//   cap         more than max_nn neighbours (max_nn != 0): the max_nn smallest (d2, packed key) are kept
//   moments     over the kept neighbours in walk order:  s += u,  P += (xx, xy, xz, yy, yz, zz) of u
//               m = s / double(n)     E = P / double(n)     C = E - (m.x*m.x, m.x*m.y, ...)
//   normal      a unit eigenvector of C for its smallest eigenvalue (cyclic Jacobi: + - * / sqrt only),
//               signed towards the viewpoint, or so that its component of largest magnitude is positive
//   curvature   max(l0, 0) / (C.xx + C.yy + C.zz), l0 = n^T C n; 0 when the trace is <= 0
//   n < 3       normal (0, 0, 1), curvature 0 (the count tells the caller)
// Every line of floating-point arithmetic is ONE IEEE float64 operation, never contracted.
#pragma once
#include <math.h>
#include <stdint.h>

#include "voxel_core.hpp"

namespace mc {

constexpr int32_t kNormalsMaxR = 4;      // radius <= 4 h: a window of at most 9^3 cells
constexpr int32_t kNormalsMinNN = 3;     // max_nn is 0 (no cap) or in [3, 64]
constexpr int32_t kNormalsMaxNN = 64;
constexpr int kNormalsCent = 4;          // float64 words per centroid record: cx, cy, cz, unused
constexpr int kNormalsSweeps = 16;       // Jacobi sweeps at most (a 3x3 converges in 4 to 6)

// the live voxel build as the search reads it: the key table, the voxel of each slot that holds a key,
// and voxel_finalise's centroids by voxel
struct NormalsGrid {
  const unsigned long long* keys;
  const uint32_t* vid;
  const double* cent;
  int shift;
  uint32_t mask;
};

struct NormalsQuery {
  int32_t R;        // ceil(radius / h), 1 .. kNormalsMaxR
  int32_t max_nn;   // 0: no cap
  double r2;        // radius * radius
};

struct NormalsMoments {
  double s[3];
  double P[6];
};

// the voxel of a key: the probe sequence of the build, until the key (true) or an empty slot (false)
MC_CORE_HD bool normals_find(const NormalsGrid& g, uint64_t key, uint32_t* v) {
  uint32_t at = voxel_slot_first(key, g.shift, g.mask);
  for (;;) {
    const uint64_t cur = g.keys[at];
    if (cur == key) {
      *v = g.vid[at];
      return true;
    }
    if (cur == kVoxelEmpty) return false;
    at = voxel_slot_next(at, g.mask);
  }
}

// fn(ix, v, u, d2) for every neighbour of the voxel at cell ki with centroid ci, in walk order; ix is the
// cell's place in the window, ((dkx + R) (2R + 1) + dky + R) (2R + 1) + dkz + R, which ascends with the
// packed key; v is the neighbour's voxel id (what the clustering of cluster_core.hpp needs beside it).  The walk
// kFromCell: the walk starts at the cell of place `first`; planes, rows and cells before it are not probed.
// skip: a walker may leave out a plane (its kx), a row (kx, ky) or a cell (kx, ky, kz) that cannot matter to it
// (register_core.hpp's nearest-centroid search); NormalsNoSkip leaves nothing out.
struct NormalsNoSkip {
  MC_CORE_HD bool plane(int32_t) const { return false; }
  MC_CORE_HD bool row(int32_t, int32_t) const { return false; }
  MC_CORE_HD bool cell(const int32_t*) const { return false; }
};

template <bool kFromCell = false, typename Fn, typename Skip = NormalsNoSkip>
MC_CORE_HD void normals_neighbours_v(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                      Fn&& fn, int32_t first = 0, const Skip& skip = Skip()) {
  MC_CORE_NO_CONTRACT
  const int32_t W = 2 * q.R + 1;
  int32_t ix = 0;
  for (int32_t dx = -q.R; dx <= q.R; ++dx) {
    int32_t k[3];
    k[0] = ki[0] + dx;
    if ((kFromCell && ix + W * W <= first) || k[0] < kVoxelKeyMin || k[0] >= kVoxelKeyEnd || skip.plane(k[0])) { ix += W * W; continue; }
    for (int32_t dy = -q.R; dy <= q.R; ++dy) {
      k[1] = ki[1] + dy;
      if ((kFromCell && ix + W <= first) || k[1] < kVoxelKeyMin || k[1] >= kVoxelKeyEnd || skip.row(k[0], k[1])) { ix += W; continue; }
      for (int32_t dz = -q.R; dz <= q.R; ++dz, ++ix) {
        k[2] = ki[2] + dz;
        if ((kFromCell && ix < first) || k[2] < kVoxelKeyMin || k[2] >= kVoxelKeyEnd || skip.cell(k)) continue;
        uint32_t v;
        if (!normals_find(g, voxel_pack(k), &v)) continue;
        const double* cj = g.cent + (int64_t)kNormalsCent * v;
        double u[3];
        u[0] = cj[0] - ci[0];
        u[1] = cj[1] - ci[1];
        u[2] = cj[2] - ci[2];
        const double xx = u[0] * u[0];
        const double yy = u[1] * u[1];
        const double zz = u[2] * u[2];
        const double xy = xx + yy;
        const double d2 = xy + zz;
        if (d2 <= q.r2) fn(ix, v, u, d2);
      }
    }
  }
}

// the same without the neighbour's id: fn(ix, u, d2)
template <typename Fn>
MC_CORE_HD void normals_neighbours(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                    Fn&& fn) {
  normals_neighbours_v(g, ki, ci, q, [&](int32_t ix, uint32_t, const double u[3], double d2) { fn(ix, u, d2); });
}

MC_CORE_HD void normals_clear(NormalsMoments* m) {
  for (int c = 0; c < 3; ++c) m->s[c] = 0.0;
  for (int c = 0; c < 6; ++c) m->P[c] = 0.0;
}

MC_CORE_HD void normals_add(NormalsMoments* m, const double u[3]) {
  MC_CORE_NO_CONTRACT
  m->s[0] = m->s[0] + u[0];
  m->s[1] = m->s[1] + u[1];
  m->s[2] = m->s[2] + u[2];
  const double xx = u[0] * u[0];
  const double xy = u[0] * u[1];
  const double xz = u[0] * u[2];
  const double yy = u[1] * u[1];
  const double yz = u[1] * u[2];
  const double zz = u[2] * u[2];
  m->P[0] = m->P[0] + xx;
  m->P[1] = m->P[1] + xy;
  m->P[2] = m->P[2] + xz;
  m->P[3] = m->P[3] + yy;
  m->P[4] = m->P[4] + yz;
  m->P[5] = m->P[5] + zz;
}

// (d2, ix) before (e2, jx): the order of the cap
MC_CORE_HD bool normals_before(double d2, int32_t ix, double e2, int32_t jx) {
  return d2 < e2 || (d2 == e2 && ix < jx);
}

// The common pass: the neighbours found, and the moments of the first max_nn of them (all of them
// without a cap).  A return above max_nn != 0 means the cap applies and *m is not the answer.
MC_CORE_HD int32_t normals_gather(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                   NormalsMoments* m) {
  int32_t found = 0;
  normals_clear(m);
  normals_neighbours(g, ki, ci, q, [&](int32_t, const double u[3], double) {
    ++found;
    if (q.max_nn == 0 || found <= q.max_nn) normals_add(m, u);
  });
  return found;
}

// The cap, first pass: the (d2, ix) of the last neighbour kept, through a list of max_nn entries
// (entry e at list[e * stride]) that holds the max_nn smallest seen so far.
MC_CORE_HD void normals_select(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                double* list_d2, uint16_t* list_ix, int32_t stride, double* last_d2, int32_t* last_ix) {
  int32_t have = 0, worst = 0;
  normals_neighbours(g, ki, ci, q, [&](int32_t ix, const double*, double d2) {
    if (have < q.max_nn) {
      list_d2[have * stride] = d2;
      list_ix[have * stride] = (uint16_t)ix;
      if (normals_before(list_d2[worst * stride], list_ix[worst * stride], d2, ix)) worst = have;
      ++have;
    } else if (normals_before(d2, ix, list_d2[worst * stride], list_ix[worst * stride])) {
      list_d2[worst * stride] = d2;
      list_ix[worst * stride] = (uint16_t)ix;
      for (int32_t e = 0; e < have; ++e)
        if (normals_before(list_d2[worst * stride], list_ix[worst * stride], list_d2[e * stride], list_ix[e * stride]))
          worst = e;
    }
  });
  *last_d2 = list_d2[worst * stride];
  *last_ix = list_ix[worst * stride];
}

// The cap, second pass: the moments of the neighbours up to (last_d2, last_ix), in walk order; -> kept
MC_CORE_HD int32_t normals_gather_capped(const NormalsGrid& g, const int32_t ki[3], const double ci[3],
                                          const NormalsQuery& q, double last_d2, int32_t last_ix, NormalsMoments* m) {
  int32_t kept = 0;
  normals_clear(m);
  normals_neighbours(g, ki, ci, q, [&](int32_t ix, const double u[3], double d2) {
    if (!normals_before(last_d2, last_ix, d2, ix)) {
      ++kept;
      normals_add(m, u);
    }
  });
  return kept;
}

// C = xx, xy, xz, yy, yz, zz of n >= 1 kept neighbours
MC_CORE_HD void normals_covariance(const NormalsMoments& m, int32_t n, double C[6]) {
  MC_CORE_NO_CONTRACT
  const double dn = (double)n;
  const double mx = m.s[0] / dn;
  const double my = m.s[1] / dn;
  const double mz = m.s[2] / dn;
  const double e0 = m.P[0] / dn;
  const double e1 = m.P[1] / dn;
  const double e2 = m.P[2] / dn;
  const double e3 = m.P[3] / dn;
  const double e4 = m.P[4] / dn;
  const double e5 = m.P[5] / dn;
  const double q0 = mx * mx;
  const double q1 = mx * my;
  const double q2 = mx * mz;
  const double q3 = my * my;
  const double q4 = my * mz;
  const double q5 = mz * mz;
  C[0] = e0 - q0;
  C[1] = e1 - q1;
  C[2] = e2 - q2;
  C[3] = e3 - q3;
  C[4] = e4 - q4;
  C[5] = e5 - q5;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3: app, aqq, apq its entries there, arp, arq
// those of the third row, v.p / v.q the eigenvector columns.  From the fourth sweep an off-diagonal
// entry below 2^-53 / 100 of both its diagonal entries is set to zero.
MC_CORE_HD void normals_rotate(int sweep, double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  MC_CORE_NO_CONTRACT
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  const double ap = fabs(app);
  const double aq = fabs(aqq);
  const double gp = ap + g;
  const double gq = aq + g;
  if (sweep >= 3 && gp == ap && gq == aq) {
    apq = 0.0;
    return;
  }
  const double h = aqq - app;
  const double ah = fabs(h);
  const double gh = ah + g;
  double t;
  if (gh == ah) {
    t = apq / h;
  } else {
    const double hh = 0.5 * h;
    const double theta = hh / apq;
    const double tt = theta * theta;
    const double t1 = tt + 1.0;
    const double rt = sqrt(t1);
    const double at = fabs(theta);
    const double den = at + rt;
    t = 1.0 / den;
    if (theta < 0.0) t = -t;
  }
  const double t2 = t * t;
  const double c1 = t2 + 1.0;
  const double cr = sqrt(c1);
  const double c = 1.0 / cr;
  const double s = t * c;
  const double d = t * apq;
  app = app - d;
  aqq = aqq + d;
  apq = 0.0;
  const double a1 = c * arp;
  const double a2 = s * arq;
  const double a3 = s * arp;
  const double a4 = c * arq;
  arp = a1 - a2;
  arq = a3 + a4;
  const double b1 = c * v0p;
  const double b2 = s * v0q;
  const double b3 = s * v0p;
  const double b4 = c * v0q;
  v0p = b1 - b2;
  v0q = b3 + b4;
  const double c2 = c * v1p;
  const double c3 = s * v1q;
  const double c4 = s * v1p;
  const double c5 = c * v1q;
  v1p = c2 - c3;
  v1q = c4 + c5;
  const double d1 = c * v2p;
  const double d2 = s * v2q;
  const double d3 = s * v2p;
  const double d4 = c * v2q;
  v2p = d1 - d2;
  v2q = d3 + d4;
}

// a unit eigenvector of C for its smallest eigenvalue (ties: the lowest Jacobi column)
MC_CORE_HD void normals_eigenvector(const double C[6], double nrm[3]) {
  MC_CORE_NO_CONTRACT
  double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < kNormalsSweeps; ++sweep) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    normals_rotate(sweep, a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    normals_rotate(sweep, a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    normals_rotate(sweep, a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  const bool one = a11 < a00;
  const double low = one ? a11 : a00;
  const bool two = a22 < low;
  const double x = two ? v02 : (one ? v01 : v00);
  const double y = two ? v12 : (one ? v11 : v10);
  const double z = two ? v22 : (one ? v21 : v20);
  const double xx = x * x;
  const double yy = y * y;
  const double zz = z * z;
  const double xy = xx + yy;
  const double l2 = xy + zz;
  const double l = sqrt(l2);
  nrm[0] = x / l;
  nrm[1] = y / l;
  nrm[2] = z / l;
}

// out = nx, ny, nz, curvature of a voxel with centroid ci, n kept neighbours and covariance C;
// has_viewpoint: signed towards (vx, vy, vz); else the canonical sign
MC_CORE_HD void normals_finish(const double C[6], int32_t n, const double ci[3], bool has_viewpoint, double vx, double vy,
                               double vz, double out[4]) {
  MC_CORE_NO_CONTRACT
  if (n < 3) {
    out[0] = 0.0;
    out[1] = 0.0;
    out[2] = 1.0;
    out[3] = 0.0;
    return;
  }
  double e[3];
  normals_eigenvector(C, e);
  bool flip;
  if (has_viewpoint) {
    const double wx = vx - ci[0];
    const double wy = vy - ci[1];
    const double wz = vz - ci[2];
    const double px = e[0] * wx;
    const double py = e[1] * wy;
    const double pz = e[2] * wz;
    const double pxy = px + py;
    const double dot = pxy + pz;
    flip = dot < 0.0;
  } else {
    double big = e[0];
    if (fabs(e[1]) > fabs(big)) big = e[1];
    if (fabs(e[2]) > fabs(big)) big = e[2];
    flip = big < 0.0;
  }
  if (flip) {
    e[0] = -e[0];
    e[1] = -e[1];
    e[2] = -e[2];
  }
  // l0 = e^T C e
  const double r0a = C[0] * e[0];
  const double r0b = C[1] * e[1];
  const double r0c = C[2] * e[2];
  const double r0d = r0a + r0b;
  const double r0 = r0d + r0c;
  const double r1a = C[1] * e[0];
  const double r1b = C[3] * e[1];
  const double r1c = C[4] * e[2];
  const double r1d = r1a + r1b;
  const double r1 = r1d + r1c;
  const double r2a = C[2] * e[0];
  const double r2b = C[4] * e[1];
  const double r2c = C[5] * e[2];
  const double r2d = r2a + r2b;
  const double r2 = r2d + r2c;
  const double l0a = e[0] * r0;
  const double l0b = e[1] * r1;
  const double l0c = e[2] * r2;
  const double l0d = l0a + l0b;
  const double l0 = l0d + l0c;
  const double tr1 = C[0] + C[3];
  const double tr = tr1 + C[5];
  const double top = l0 > 0.0 ? l0 : 0.0;
  out[0] = e[0];
  out[1] = e[1];
  out[2] = e[2];
  out[3] = tr > 0.0 ? top / tr : 0.0;
}

// ---- kept normals: the voxels an edit of the cloud makes stale (include/mcdeskew.h "kept normals") -------------------
// The estimate of a voxel reads the occupied cells of its window and their centroids and nothing else, and the window
// relation is symmetric: the rows an edit can change are those of the voxels in the window of a touched cell.  Every
// voxel carries a 32-bit stamp; an edit has an epoch, and the first lane that exchanges the epoch into a voxel's stamp
// has claimed the voxel for this edit.  Nothing is cleared per edit: an older stamp is simply not the epoch.  0 is never
// an epoch (fresh stamps are 0), and the edit after epoch 2^32 - 1 clears the stamps and starts again at 1.
constexpr uint32_t kNormalsEpochLast = 0xFFFFFFFFu;

// the epoch of the edit after the one of `epoch` (0: none yet); *clear: the stamps go back to 0 first
MC_CORE_HD uint32_t normals_next_epoch(uint32_t epoch, bool* clear) {
  *clear = epoch == kNormalsEpochLast;
  return *clear ? 1u : epoch + 1u;
}

// whether this is the edit's first claim of voxel v.  Stamps: exchange(v, epoch) -> the word before (the device's
// atomicExch; a harness's plain swap)
template <typename Stamps>
MC_CORE_HD bool normals_claim(Stamps& stamps, uint32_t v, uint32_t epoch) {
  return stamps.exchange(v, epoch) != epoch;
}

// fn(v) for every voxel in the (2R + 1)^3 window of cell ki that this edit claims here first, in walk order; cells
// outside the key range do not exist, as in normals_neighbours_v.  The centroids of g are not read
template <typename Stamps, typename Fn>
MC_CORE_HD void normals_mark_window(const NormalsGrid& g, const int32_t ki[3], int32_t R, uint32_t epoch, Stamps& dirty,
                                     Fn&& fn) {
  for (int32_t dx = -R; dx <= R; ++dx) {
    int32_t k[3];
    k[0] = ki[0] + dx;
    if (k[0] < kVoxelKeyMin || k[0] >= kVoxelKeyEnd) continue;
    for (int32_t dy = -R; dy <= R; ++dy) {
      k[1] = ki[1] + dy;
      if (k[1] < kVoxelKeyMin || k[1] >= kVoxelKeyEnd) continue;
      for (int32_t dz = -R; dz <= R; ++dz) {
        k[2] = ki[2] + dz;
        if (k[2] < kVoxelKeyMin || k[2] >= kVoxelKeyEnd) continue;
        uint32_t v;
        if (normals_find(g, voxel_pack(k), &v) && normals_claim(dirty, v, epoch)) fn(v);
      }
    }
  }
}

}  // namespace mc
