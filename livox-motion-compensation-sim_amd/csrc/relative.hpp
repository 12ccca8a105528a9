// relative.hpp — the SLERP deskew into the sensor frame at a per-frame reference time
// (mc_deskew_relative, build-added like SURVEY §8a a11):
//   p' = R_ref^T (R(q(t)) p + pos(t) - pos_ref),  (R_ref, pos_ref) = the SLERP / LERP pose at t_ref[f].
//
//   k_pose_at             the pose the library interpolates at arbitrary times (mc_pose_at, and the
//                         reference poses of the two relative entries);
//   k_rel_count           per frame, the true width of its segment window [klo, khi] (FrameWin::W
//                         saturates at kWinMax + 1), which sizes the per-frame relative table;
//   k_rel_compose         after k_prep: every record of every frame's [klo, khi], folded into the
//                         frame's reference pose (relfold.hpp) and specialised to the frame time.
// The deskew itself is k_deskew_points<1, false, false, RULE, RelArgs> (kernels.hpp): the global kernel with
// every record read from that per-frame table; the float64 rows by the direct formula are
// k_points_f64<1, RefPoses>.
#pragma once
#include "kernels.hpp"

namespace mc {

struct PoseAtArgs {
  const double* t; int64_t n;                              // query times (s, the pose table's base)
  const double* pose_time; const PoseSeg* pose_seg; int64_t nseg; int64_t ntab;
  double* R;     // (n, 3, 3) row-major, or null
  double* pos;   // (n, 3), or null
  double* q;     // (n, 4) (x, y, z, w), or null
};

// One thread per time: the segment, alpha, then the quaternion and position exactly as slerp_core
// forms them (general tier), R = I + 2 (w [u]x + [u]x^2) of that quaternion (slerp_core's rotation).
__global__ __launch_bounds__(kBlock) void k_pose_at(const PoseAtArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    const double tq = a.t[i];
    const PoseSeg s = a.pose_seg[pose_segment_of(a.pose_time, a.ntab, a.nseg, tq)];
    double al = (tq - s.t0) * s.inv_dt;
    al = fmin(fmax(al, 0.0), 1.0);
    double cs, sc;
    cos_sinc(kPoly10, al * s.th, cs, sc);
    const double sn = al * sc;
    const double x = fma(sn, s.v[0], cs * s.q0[0]), y = fma(sn, s.v[1], cs * s.q0[1]);
    const double z = fma(sn, s.v[2], cs * s.q0[2]), w = fma(sn, s.v[3], cs * s.q0[3]);
    if (a.q) {
      double* o = a.q + 4 * i;
      o[0] = x; o[1] = y; o[2] = z; o[3] = w;
    }
    if (a.pos) {
      double* o = a.pos + 3 * i;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = fma(al, s.dp[c], s.p0[c]);
    }
    if (a.R) {
      double* o = a.R + 9 * i;
      o[0] = 1.0 - 2.0 * (y * y + z * z); o[1] = 2.0 * (x * y - z * w);       o[2] = 2.0 * (x * z + y * w);
      o[3] = 2.0 * (x * y + z * w);       o[4] = 1.0 - 2.0 * (x * x + z * z); o[5] = 2.0 * (y * z - x * w);
      o[6] = 2.0 * (x * z - y * w);       o[7] = 2.0 * (y * z + x * w);       o[8] = 1.0 - 2.0 * (x * x + y * y);
    }
  }
}

// [klo, khi] of frame f from its t_ns span, as prep_body<1> selects it
__device__ __forceinline__ void frame_segments(const double* time, int64_t T, int64_t nseg, double tf, int2 tr,
                                               int64_t* klo, int64_t* khi) {
  *klo = *khi = 0;
  if (tr.x <= tr.y) {
    *klo = pose_segment_of(time, T, nseg, slerp_time(tf, (double)tr.x));
    *khi = pose_segment_of(time, T, nseg, slerp_time(tf, (double)tr.y));
  }
}

struct RelTableArgs {
  int32_t F;
  const double* frame_time; const int2* trange;
  const double* pose_time; int64_t T; int64_t nseg;
  int32_t* width;           // k_rel_count: khi - klo + 1 per frame (>= 1)
  // k_rel_compose
  const int64_t* roff;      // first record of frame f in the relative table (F + 1 entries)
  const PoseSeg* pose_seg;  // the step's segment table (k_prep)
  const double* ref_q;      // (F, 4) reference quaternion, (F, 3) reference position (k_pose_at)
  const double* ref_pos;
  PoseWin* rel;             // roff[F] records
};

__global__ __launch_bounds__(kBlock) void k_rel_count(const RelTableArgs a) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= a.F) return;
  int64_t klo, khi;
  frame_segments(a.pose_time, a.T, a.nseg, a.frame_time[f], a.trange[f], &klo, &khi);
  a.width[f] = (int32_t)(khi - klo + 1);
}

// One thread per record of the relative table: record j of frame f = segment klo_f + j of the step's
// table, folded into the frame's reference pose, with the frame's time (a PoseWin).
__global__ __launch_bounds__(kBlock) void k_rel_compose(const RelTableArgs a) {
  const int64_t total = a.roff[a.F];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int32_t f = row_frame(a.roff, a.F, i);
    const double tf = a.frame_time[f];
    int64_t klo, khi;
    frame_segments(a.pose_time, a.T, a.nseg, tf, a.trange[f], &klo, &khi);
    int64_t k = klo + (i - a.roff[f]);
    k = k > a.nseg - 1 ? a.nseg - 1 : k;
    PoseWin w = a.pose_seg[k];
    const double* rq = a.ref_q + 4 * (int64_t)f;
    const double* rp = a.ref_pos + 3 * (int64_t)f;
    const double qr[4] = {rq[0], rq[1], rq[2], rq[3]}, pr[3] = {rp[0], rp[1], rp[2]};
    rel_fold(qr, pr, w.q0, w.v, w.p0, w.dp);
    w.tf = tf;
    a.rel[i] = w;
  }
}

}  // namespace mc
