// plane.hpp — the kernels of the voxel cloud's plane segmentation and of the selection of a subset of the cloud
// into a batch (host side in voxel.hip; scalar core in plane_core.hpp).  They read the live voxel build: the
// centroids by voxel id (normals.hpp) and, for the selection, what the emit kernels read.
//
//   compact   a mask's set bytes flagged per workgroup, scanned (k_vox_scan) and scattered: ids[rank] = voxel id,
//             ascending.  The candidates of a segmentation with `among`, and the voxels of a selection
//   sample    one lane per hypothesis: the three samples and the 64-byte record n, d, tau, p0
//   score     K n point-plane tests.  A lane keeps kPlanePts centroids in registers and loops over a chunk of
//             kPlaneChunk hypotheses, read through the scalar unit (the record is wave-uniform); per hypothesis
//             the wave's inliers are a ballot and a popcount per centroid, added once into the workgroup's LDS
//             counter; a workgroup walks its tiles with the counters in LDS and adds them to score[K] at its
//             end with 32-bit integer atomics.  More than kPlaneChunk hypotheses: further launches
//   mask      the inlier byte per voxel under a hypothesis or under the refined model, and their number
//   moments   the nine tree sums: per workgroup of 256 leaves an xor-butterfly inside each wave (adjacent pairs:
//             float64 addition commutes), then the four waves' sums pairwise; the next level reads the level
//             before as its leaves, and the last fewer than 256 partials are summed by the host the same way
//   select    k_vox_emit_batch's values for the voxels ids[0 .. n)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_core.hpp"
#include "voxel.hpp"

namespace mc {

constexpr int kPlaneChunk = 1024;    // hypotheses per score launch: the workgroup's LDS counters (4 KB)
constexpr int kPlanePts = 4;         // centroids per lane of the score kernel
constexpr int kPlaneTile = kVoxBlock * kPlanePts;   // voxels per workgroup and turn
constexpr int kPlaneScoreGrid = 2048;               // workgroups at most: 8 per CU

// per workgroup of kVoxBlock voxels: the number of set mask bytes
__global__ __launch_bounds__(kVoxBlock) void k_pl_flag(const uint8_t* mask, int64_t M, uint32_t* chunk_count) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  const uint32_t on = v < M && mask[v] != 0 ? 1u : 0u;
  uint32_t excl;
  const uint32_t total = vox_block_scan(on, &excl);
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// ids[rank] = v for every set byte (chunk_off: the scanned counts); rank < the scan's total <= M
__global__ __launch_bounds__(kVoxBlock) void k_pl_scatter(const uint8_t* mask, int64_t M, const uint32_t* chunk_off,
                                                          uint32_t* ids) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  const uint32_t on = v < M && mask[v] != 0 ? 1u : 0u;
  uint32_t excl;
  vox_block_scan(on, &excl);
  if (on) ids[chunk_off[blockIdx.x] + excl] = (uint32_t)v;
}

struct PlaneSampleArgs {
  const double* cent;     // the centroids by voxel id
  const uint32_t* ids;    // the n candidates, ascending; null: the identity
  int64_t n;              // >= 3
  uint64_t seed;
  int32_t K;
  double tt;              // t * t
  double* hyp;            // K records of kPlaneHyp words
  int32_t* samples;       // K x 3 voxel ids
};

__global__ __launch_bounds__(kVoxBlock) void k_pl_sample(PlaneSampleArgs a) {
  const int32_t k = (int32_t)(blockIdx.x * kVoxBlock + threadIdx.x);
  if (k >= a.K) return;
  uint64_t at[3];
  plane_sample(a.seed, (uint32_t)k, (uint64_t)a.n, at);
  double p[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint32_t v = a.ids ? a.ids[at[j]] : (uint32_t)at[j];   // at[j] < n
    a.samples[3 * k + j] = (int32_t)v;
    const double* c = a.cent + (int64_t)kNormalsCent * v;
    p[j][0] = c[0];
    p[j][1] = c[1];
    p[j][2] = c[2];
  }
  const PlaneHyp h = plane_hypothesis(p[0], p[1], p[2], a.tt);
  double2* o = reinterpret_cast<double2*>(a.hyp + (int64_t)kPlaneHyp * k);
  o[0] = make_double2(h.n[0], h.n[1]);
  o[1] = make_double2(h.n[2], h.d);
  o[2] = make_double2(h.tau, h.p0[0]);
  o[3] = make_double2(h.p0[1], h.p0[2]);
}

// the five words of a record the tests read
struct PlaneTest {
  double nx, ny, nz, d, tau;
};

// score[k0 + k] += the candidates inside hypothesis k0 + k, k < kn <= kPlaneChunk
__global__ __launch_bounds__(kVoxBlock) void k_pl_score(const double* cent, const uint8_t* among, int64_t M,
                                                        const double* hyp, int32_t k0, int32_t kn, uint32_t* score) {
  __shared__ uint32_t inside[kPlaneChunk];
  for (int k = threadIdx.x; k < kn; k += kVoxBlock) inside[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t tiles = (M + kPlaneTile - 1) / kPlaneTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // a voxel that is no candidate (or past the end) is held as NaN: its s is NaN and s * s <= tau is false
    double cx[kPlanePts], cy[kPlanePts], cz[kPlanePts];
#pragma unroll
    for (int j = 0; j < kPlanePts; ++j) {
      const int64_t v = tile * kPlaneTile + j * kVoxBlock + threadIdx.x;
      const bool on = v < M && (!among || among[v] != 0);
      const double2* c = reinterpret_cast<const double2*>(cent + kNormalsCent * (v < M ? v : 0));
      const double2 xy = c[0];
      cx[j] = on ? xy.x : __builtin_nan("");
      cy[j] = xy.y;
      cz[j] = c[1].x;
    }
    const PlaneTest* rec = reinterpret_cast<const PlaneTest*>(hyp + (int64_t)kPlaneHyp * k0);
    PlaneTest next = ldu(rec);
    for (int k = 0; k < kn; ++k) {
      const PlaneTest h = next;
      // the record after this one, asked for before this one's tests (the last turn reads its own again)
      next = ldu(reinterpret_cast<const PlaneTest*>(reinterpret_cast<const double*>(rec) + kPlaneHyp * (k + 1 < kn ? k + 1 : k)));
      uint32_t wave = 0;
#pragma unroll
      for (int j = 0; j < kPlanePts; ++j) {
        const bool in = plane_inlier(h.nx, h.ny, h.nz, h.d, h.tau, cx[j], cy[j], cz[j]);
        wave += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
      }
      if (wave && lane == 0) atomicAdd(&inside[k], wave);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kn; k += kVoxBlock)
    if (inside[k]) atomicAdd(score + k0 + k, inside[k]);
}

struct PlaneMaskArgs {
  const double* cent;
  const uint8_t* among;   // null: every voxel is a candidate
  int64_t M;
  double n[3], d;
  double bound;           // tau (refined 0) or t (refined 1)
  int32_t refined;
  uint8_t* mask;          // (M,)
  uint32_t* count;        // [0] += the inliers
};

__global__ __launch_bounds__(kVoxBlock) void k_pl_mask(PlaneMaskArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  bool in = false;
  if (v < a.M && (!a.among || a.among[v] != 0)) {
    const double* c = a.cent + kNormalsCent * v;
    in = a.refined ? plane_within(a.n[0], a.n[1], a.n[2], a.d, a.bound, c[0], c[1], c[2])
                   : plane_inlier(a.n[0], a.n[1], a.n[2], a.d, a.bound, c[0], c[1], c[2]);
  }
  if (v < a.M) a.mask[v] = in ? 1 : 0;
  const uint32_t wave = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
  if ((threadIdx.x & 63) == 0 && wave) atomicAdd(a.count, wave);
}

// the sums of the workgroup's 256 leaves of kW values each as the adjacent-pair tree gives them (every thread takes
// part); thread c < kW stores sum c.  kW = kPlaneSums: the refit's; kRegSums: the registration's (register.hpp)
template <int kW>
__device__ __forceinline__ void plane_block_tree(double x[kW], double* out, int64_t out_stride) {
  __shared__ double part[kVoxBlock / 64][kW];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int c = 0; c < kW; ++c) x[c] = x[c] + __shfl_xor(x[c], d, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kW; ++c) part[wave][c] = x[c];
  }
  __syncthreads();
  if (threadIdx.x < kW) {
    const int c = threadIdx.x;
    const double lo = part[0][c] + part[1][c];
    const double hi = part[2][c] + part[3][c];
    out[c * out_stride] = lo + hi;
  }
}

// the first level: leaves 256 b .. 256 b + 255 of the voxels' nine values -> out[c * gridDim.x + b]
__global__ __launch_bounds__(kVoxBlock) void k_pl_moments(const double* cent, const uint8_t* mask, int64_t M, double p0x,
                                                          double p0y, double p0z, double* out) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  double x[kPlaneSums];
  const bool in = v < M && mask[v] != 0;
  const double* cv = cent + kNormalsCent * (v < M ? v : 0);
  const double c[3] = {cv[0], cv[1], cv[2]}, p0[3] = {p0x, p0y, p0z};
  plane_leaf(in, c, p0, x);
  plane_block_tree<kPlaneSums>(x, out + blockIdx.x, gridDim.x);
}

// a further level of a tree of kW sums: in[c * count + i], count = 256 gridDim.x -> out[c * gridDim.x + b]
template <int kW>
__global__ __launch_bounds__(kVoxBlock) void k_pl_tree(const double* in, int64_t count, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  double x[kW];
#pragma unroll
  for (int c = 0; c < kW; ++c) x[c] = in[c * count + i];
  plane_block_tree<kW>(x, out + blockIdx.x, gridDim.x);
}

// k_vox_emit_batch over the voxels ids[0 .. n): point p is voxel ids[p]
__global__ __launch_bounds__(kVoxBlock) void k_pl_emit_selected(VoxOut a, int64_t P, const uint32_t* ids, int64_t n) {
  const int64_t p0 = ((int64_t)blockIdx.x * kVoxBlock + threadIdx.x) * 4;
  if (p0 >= P) return;
  vox_emit_four(a, p0, n, [&](int64_t p) { return (int64_t)ids[p]; });
}

}  // namespace mc
