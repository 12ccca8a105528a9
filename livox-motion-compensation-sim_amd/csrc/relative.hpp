// relative.hpp — the SLERP deskew into the sensor frame at a per-frame reference time
// (mc_deskew_relative, build-added like SURVEY §8a a11):
//   p' = R_ref^T (R(q(t)) p + pos(t) - pos_ref),  (R_ref, pos_ref) = the SLERP / LERP pose at t_ref[f].
//
//   k_pose_at             the pose the library interpolates at arbitrary times (mc_pose_at, and the
//                         reference poses of the two relative entries);
//   k_rel_count           per frame, the true width of its segment window [klo, khi] (FrameWin::W
//                         saturates at kWinMax + 1), which sizes the per-frame relative table;
//   k_rel_compose         after k_prep: every record of every frame's [klo, khi], folded into the
//                         frame's reference pose (relfold.hpp) and specialised to the frame time;
//   k_deskew_points_rel   k_deskew_points<1> with every record read from that per-frame table: the
//                         per-point instruction stream (fast_path / points4 / points_peeled /
//                         slerp_point, unchanged) and the 36 B per point are the global kernel's;
//   k_points_rel_f64      float64 rows by the direct formula (global value, minus pos_ref, R_ref^T):
//                         an independent device-side check of the folded path.
#pragma once
#include "kernels.hpp"
#include "relfold.hpp"

namespace mc {

// segment of the pose table at time t as the oracle selects it: searchsorted 'right' - 1, clamped
__device__ __forceinline__ int64_t pose_segment_of(const double* time, int64_t T, int64_t nseg, double t) {
  const int64_t k = upper_bound(time, T, t) - 1;
  return k > nseg - 1 ? nseg - 1 : (k < 0 ? 0 : k);
}

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

// The relative table as the deskew kernel takes it (by value, beside DeskewArgs, whose layout stays).
struct RelArgs {
  const PoseWin* rel;     // per-frame folded records of [klo_f, khi_f], frame-specialised (tf set)
  const int64_t* roff;    // F + 1 offsets into rel
};

// k_deskew_points<1> with the records of the relative table.  A frame's window [klo_f, khi_f] starts
// at rel + roff[f]; a window fw (the frame's own, or a sub-tile's) inside it starts fw.klo - klo_f
// records further on.  All four window paths read from there:
//   W <= 2      scalar loads of the folded records (never composed per wave);
//   W <= 64     the tid < W lanes copy the folded records into LDS;
//   W > 64      per-point search of the pose times, the record of segment k at k - klo_f (clamped into
//               the frame's window: a padding slot's t_ns = 0 may lie outside the valid points' span).
__global__ __launch_bounds__(kBlock, kPointsWaves) void k_deskew_points_rel(const DeskewArgs a, const RelArgs ra) {
  span_start(a.span);
  __shared__ PoseWin s_win[kWinMax];
  __shared__ int64_t s_bnd[kWinMax];
  const int tid = threadIdx.x;
  const int64_t n_sub = (int64_t)a.n_tiles * kSub;
  const uint32_t b0 = blockIdx.x, nb = gridDim.x;
  for (int64_t it = b0; it < n_sub; it += nb) {
    const int64_t st = nb < n_sub ? it : (a.xcd_order ? xcd_unit<1>(it, n_sub) : it);
    const Tile tl = ldu(a.tiles + st / kSub);
    const int g0 = (int)(st % kSub) * kBlock;
    if (g0 >= tl.ngroups) continue;  // uniform: empty sub-tile of a short tile
    // every lane loads (k_deskew_points' load_sub: idle lanes re-read the sub-tile's first group)
    const int g = g0 + tid;
    const bool act = g < tl.ngroups;
    const int gl = act ? g : g0;
    const float* q = a.in + bidx((int)a.in_C, 0, tl.pstart + 4 * (int64_t)gl);
    const int4 Tq = ld4(reinterpret_cast<const int32_t*>(q + 4 * kBlkPts));
    float4 X = ld4(q), Y = ld4(q + kBlkPts), Z = ld4(q + 2 * kBlkPts);
    const float4 I = ld4(q + 3 * kBlkPts);
    const int f = tl.frame;
    const int64_t p = tl.pstart + 4 * (int64_t)g;
    const FrameWin ff = ldu(a.fwin + f);
    const bool sub = ff.W > kFastMaxW;
    const FrameWin fw = ldu(sub ? a.swin + st : a.fwin + f);
    const int64_t r0 = ldu(ra.roff + f), r1 = ldu(ra.roff + f + 1);
    const PoseWin* frel = ra.rel + r0;             // the frame's records, segment klo_f first
    const PoseWin* rec = frel + (fw.klo - ff.klo);  // the window's
    if (fw.W <= kFastMaxW) {
      if (fw.tier == 0) fast_path<1, 0>(rec, fw, false, 0.0, act, Tq, X, Y, Z);
      else if (fw.tier == 1) fast_path<1, 1>(rec, fw, false, 0.0, act, Tq, X, Y, Z);
      else fast_path<1, kTierAny<1>>(rec, fw, false, 0.0, act, Tq, X, Y, Z);
    } else if (fw.W <= kWinMax) {
      const int W = fw.W;
      if (tid < W) {
        s_win[tid] = rec[tid];
        s_bnd[tid] = rel_ns_ceil(a.pose_time[fw.klo + tid], a.frame_time[f]);
      }
      __syncthreads();
      int seg[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) seg[c] = act ? win_index(s_bnd, W, (int64_t)i4c(Tq, c)) : -1;
      points_peeled<1>(seg, [&](int j) { return uniform_of(s_win[j]); }, poly_load<kTierAny<1>>(), Tq, X, Y, Z);
      __syncthreads();  // the LDS window is rewritten by the next sub-tile
    } else {
      const double tf = a.frame_time[f];
      const int64_t wmax = r1 - r0 - 1;   // khi_f - klo_f
      int seg[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        int64_t j = pose_segment_of(a.pose_time, a.ntab, a.nseg, slerp_time(tf, (double)i4c(Tq, c))) - ff.klo;
        j = j > wmax ? wmax : (j < 0 ? 0 : j);
        seg[c] = act ? (int)j : -1;
      }
      points_peeled<1>(seg, [&](int j) { return ldu(frel + j); }, poly_load<kTierAny<1>>(), Tq, X, Y, Z);
    }
    if (act) {
      float* o = a.out + bidx((int)a.out_C, 0, p);
      st_out(o, X);
      st_out(o + kBlkPts, Y);
      st_out(o + 2 * kBlkPts, Z);
      st_out(o + 3 * kBlkPts, I);
      if (a.copy_t) st_out(o + 4 * kBlkPts, __builtin_bit_cast(float4, Tq));
    }
  }
  span_end(a.span);
}

// ---- float64 rows, the direct formula ---------------------------------------------------------------
// Per point the global float64 value of k_points_f64<1> (slerp_core<double> on the plain segment
// record), then minus pos_ref, then R_ref^T: no folded record anywhere.
struct PointsRelF64Args {
  PointsF64Args p;
  const double* ref_q;     // (F, 4)
  const double* ref_pos;   // (F, 3)
};

__global__ __launch_bounds__(kBlock) void k_points_rel_f64(const PointsRelF64Args b) {
  const PointsF64Args& a = b.p;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    const int32_t f = row_frame(a.doff, a.F, i);
    const double* q = a.pts + i * a.ld;
    double x = q[0], y = q[1], z = q[2];
    const double w = a.ld > 3 ? q[3] : 0.0;
    const double tq = slerp_time(a.ftime[f], (double)a.t_ns[i]);
    slerp_core(a.pose_seg[pose_segment_of(a.pose_time, a.ntab, a.nseg, tq)], kPoly10, tq, x, y, z);
    const double* rq = b.ref_q + 4 * (int64_t)f;
    const double* rp = b.ref_pos + 3 * (int64_t)f;
    const double qr[4] = {rq[0], rq[1], rq[2], rq[3]};
    const double d[3] = {x - rp[0], y - rp[1], z - rp[2]};
    double o3[3];
    quat_rot_inv(qr, d, o3);
    double* o = a.out + 4 * i;
    o[0] = o3[0]; o[1] = o3[1]; o[2] = o3[2]; o[3] = w;
  }
}

}  // namespace mc
