// register.hpp — the kernels of the point-to-plane registration of a source against the voxel cloud (host side in
// voxel.hip; scalar core in register_core.hpp).  They read the live voxel build through what the normals read: the
// key table, vid and the centroids by voxel id.  A source point's index is its place in the source: the row for
// float64 rows, frame-major then the index within the frame for a batch (padding slots are not points).
//
//   correspond  one lane per source point: the point moved by the pose, its cell, the (2W + 1)^3 probes of the
//               window around it in key order and the nearest centroid within max_distance: its voxel id and d2
//   leaves      one lane per source point: the point moved again, the centroid and the normal of its voxel, its 28
//               leaves, and the first level of the tree over the point index (plane_block_tree of plane.hpp);
//               the pairs are counted with an integer atomic per wave
//   tree        the further levels: k_pl_tree<kRegSums> of plane.hpp
//
// The frames of a batch registered together (mc_voxel_register_frames): every frame a source of its own with its own
// pose, tree, pair count and stop, all of them advanced by one launch sequence per iteration; a workgroup whose frame
// has ended returns at once, so an ended frame is not written again.
//   frames step   frame f owns plane_leaves(n_f) / 256 consecutive workgroups (the block map boff, searched in scalar
//                 registers); one lane per point: correspond and leaves in one, the point moved once and no ids array;
//                 the first level of the frame's tree.  Workgroups past the frame's last point leave their partials
//                 as the call zeroed them
//   frames tree   a further level of every frame that has one, one launch per level (a block map per level)
//   frames solve  one workgroup per frame: the last fewer than 256 partials of the 28 sums, one lane each, then one
//                 lane's register_step, the history row and the frame's record; the frames still live are counted
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane.hpp"
#include "register_core.hpp"

namespace mc {

struct RegSrc {
  // a batch: blocked columns (layout.hpp) and its F + 1 padded and dense offsets
  const float* cols;
  int32_t C, F;
  const int64_t* poff;
  const int64_t* doff;
  // float64 rows x, y, z, ...
  const double* rows;
  int64_t ld;
  int64_t first;   // the source's first point among the batch's dense points (a single frame: its offset)
  int64_t n;       // points of the source
};

struct RegArgs {
  RegSrc src;
  RegPose T;
  NormalsGrid g;
  int64_t M;
  double h, o[3];
  NormalsQuery w;
  int32_t* ids;               // (n,) the nearest voxel, -1: none
  double* d2;                 // (n,) or null
  const double* normals;      // (M, 4) the leaves' normals
  const int32_t* counts;      // (M,) the neighbours they were estimated from
  double* out;                // the tree's first level: kRegSums x gridDim.x
  unsigned long long* pairs;  // [0] += the pairs
};

// source point i < n as float64
template <bool BATCH>
__device__ __forceinline__ void reg_point(const RegSrc& s, int64_t i, double p[3]) {
  if (BATCH) {
    const int64_t d = s.first + i;
    int32_t lo = 0, hi = s.F - 1;
    while (lo < hi) {   // the last frame that starts at or before d (empty frames start where the next begins)
      const int32_t mid = (lo + hi + 1) >> 1;
      if (s.doff[mid] <= d) lo = mid;
      else hi = mid - 1;
    }
    const int64_t pp = s.poff[lo] + (d - s.doff[lo]);   // d is inside frame lo: pp < poff[lo + 1] <= P
    const float* b = s.cols + bidx(s.C, 0, pp);
    p[0] = (double)b[0];
    p[1] = (double)b[kBlkPts];
    p[2] = (double)b[2 * kBlkPts];
  } else {
    const double* r = s.rows + i * s.ld;
    p[0] = r[0];
    p[1] = r[1];
    p[2] = r[2];
  }
}

template <bool BATCH>
__global__ __launch_bounds__(kVoxBlock) void k_rg_correspond(RegArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (i >= a.src.n) return;
  double p[3], q[3];
  reg_point<BATCH>(a.src, i, p);
  register_move(a.T, p, q);
  int32_t id = -1;
  double d2 = (double)INFINITY;
  if (a.M > 0) register_nearest(a.g, a.h, a.o, a.w, q, &id, &d2);
  a.ids[i] = id;
  if (a.d2) a.d2[i] = d2;
}

// the first level: leaves 256 b .. 256 b + 255 of the source points' 28 values -> out[c * gridDim.x + b]
template <bool BATCH>
__global__ __launch_bounds__(kVoxBlock) void k_rg_leaves(RegArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  double q[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
  bool pair = false;
  if (i < a.src.n) {
    const int32_t id = a.ids[i];
    if (id >= 0 && a.counts[id] >= kNormalsMinNN) {   // 0 <= id < M: the correspondence kernel's
      double p[3];
      reg_point<BATCH>(a.src, i, p);
      register_move(a.T, p, q);
      const double* cv = a.g.cent + (int64_t)kNormalsCent * id;
      const double* nv = a.normals + 4 * (int64_t)id;
      c[0] = cv[0]; c[1] = cv[1]; c[2] = cv[2];
      n[0] = nv[0]; n[1] = nv[1]; n[2] = nv[2];
      pair = true;
    }
  }
  double x[kRegSums];
  register_leaf(pair, q, c, n, x);
  const uint32_t wave = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pair));
  if ((threadIdx.x & 63) == 0 && wave) atomicAdd(a.pairs, (unsigned long long)wave);
  plane_block_tree<kRegSums>(x, a.out + blockIdx.x, gridDim.x);
}

static_assert(kRegBlock == kVoxBlock, "a workgroup is a node of the tree");

struct RegFramesArgs {
  const float* cols;          // the batch's blocked columns
  int32_t C, F;
  const int64_t* poff;        // (F + 1,) the frames' padded offsets
  const int64_t* boff;        // (F + 1,) the block map of the launch
  RegFrame* fr;               // (F,)
  NormalsGrid g;
  int64_t M;
  double h, o[3];
  NormalsQuery w;
  const double* normals;
  const int32_t* counts;
  double* tree;               // every frame's levels (RegFrame::tree), zeroed once per call
  int32_t level;              // k_rg_frames_tree: the level written (2: the second)
  int32_t max_iterations;
  double tol_rotation, tol_translation;
  double* history;            // (F, max_iterations, kRegHistory), zeroed once per call
  uint32_t* live;             // [0] += the frames that go on
};

__global__ __launch_bounds__(kVoxBlock) void k_rg_frames_step(RegFramesArgs a) {
  const int64_t b = blockIdx.x;
  const int32_t f = register_block_frame(a.boff, a.F, b);   // of blockIdx alone: wave-uniform
  const RegFrame* fr = a.fr + f;
  // the record through the scalar unit: nothing here but `count` is written while this kernel runs
  if (ldu(&fr->status) != kRegGoOn) return;
  const int64_t lb = b - a.boff[f], n = ldu(&fr->n);         // 0 <= lb < fr->blocks
  if (lb * kVoxBlock >= n) return;                           // no point here: the partials stay +0.0
  const RegPose T = ldu(&fr->T);
  const int64_t i = lb * kVoxBlock + threadIdx.x;
  double q[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
  bool pair = false;
  if (i < n) {
    const float* src = a.cols + bidx(a.C, 0, a.poff[f] + i);   // i < n: inside frame f's padded span
    const double p[3] = {(double)src[0], (double)src[kBlkPts], (double)src[2 * kBlkPts]};
    register_move(T, p, q);
    int32_t id = -1;
    double d2;
    if (a.M > 0) register_nearest(a.g, a.h, a.o, a.w, q, &id, &d2);
    if (id >= 0 && a.counts[id] >= kNormalsMinNN) {            // 0 <= id < M: a voxel of the table
      const double* cv = a.g.cent + (int64_t)kNormalsCent * id;
      const double* nv = a.normals + 4 * (int64_t)id;
      c[0] = cv[0]; c[1] = cv[1]; c[2] = cv[2];
      nn[0] = nv[0]; nn[1] = nv[1]; nn[2] = nv[2];
      pair = true;
    }
  }
  double x[kRegSums];
  register_leaf(pair, q, c, nn, x);
  const uint32_t wave = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pair));
  if ((threadIdx.x & 63) == 0 && wave) atomicAdd(&a.fr[f].count, (unsigned long long)wave);
  plane_block_tree<kRegSums>(x, a.tree + ldu(&fr->tree) + lb, ldu(&fr->blocks));
}

// level a.level >= 2 of every live frame that has it: k_pl_tree<kRegSums> on the frame's own levels
__global__ __launch_bounds__(kVoxBlock) void k_rg_frames_tree(RegFramesArgs a) {
  const int64_t b = blockIdx.x;
  const int32_t f = register_block_frame(a.boff, a.F, b);
  const RegFrame* fr = a.fr + f;
  if (fr->status != kRegGoOn) return;
  int64_t cnt;
  const int64_t at = register_level(fr->blocks, a.level - 1, &cnt);   // the level read: cnt >= 256 partials per sum
  const double* in = a.tree + fr->tree + at;
  double* out = a.tree + fr->tree + at + (int64_t)kRegSums * cnt;
  const int64_t lb = b - a.boff[f];                                   // < cnt / 256
  const int64_t i = lb * kVoxBlock + threadIdx.x;
  double x[kRegSums];
#pragma unroll
  for (int c = 0; c < kRegSums; ++c) x[c] = in[c * cnt + i];
  plane_block_tree<kRegSums>(x, out + lb, cnt / kVoxBlock);
}

__global__ __launch_bounds__(kVoxBlock) void k_rg_frames_solve(RegFramesArgs a) {
  __shared__ double top[kRegSums][kRegTopMax];
  __shared__ double sums[kRegSums];
  RegFrame* fr = a.fr + blockIdx.x;
  if (fr->status != kRegGoOn) return;
  const int32_t cnt = fr->top_n;                                      // 1 .. 128, a power of two
  const double* in = a.tree + fr->top;
  for (int k = threadIdx.x; k < kRegSums * cnt; k += kVoxBlock) top[k / cnt][k % cnt] = in[k];
  __syncthreads();
  if (threadIdx.x < kRegSums) sums[threadIdx.x] = register_tail(top[threadIdx.x], cnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    RegFrame r = *fr;
    double s[kRegSums];
    for (int c = 0; c < kRegSums; ++c) s[c] = sums[c];
    const bool on = register_frame_end(&r, s, a.max_iterations, a.tol_rotation, a.tol_translation,
                                       a.history + (int64_t)blockIdx.x * a.max_iterations * kRegHistory);
    *fr = r;
    if (on) atomicAdd(a.live, 1u);
  }
}

}  // namespace mc
