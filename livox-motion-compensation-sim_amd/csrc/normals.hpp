// normals.hpp — the kernels of the voxel cloud's surface normals (host side in voxel.hip; scalar core in
// normals_core.hpp).  They read the live voxel build: its key table, vid, vslot, sums and cnt.
//
// Three phases, one lane per voxel:
//   centroids   once per build: voxel_finalise's cx, cy, cz of every voxel into a dense array by voxel id
//               (32 B records), so a probe that hits costs key -> vid -> centroid, not the 36-byte record and
//               six conversions and divisions per neighbour
//   window      the (2R + 1)^3 probes of the voxel's window in key order, accumulating the moments while it
//               probes; a voxel with at most max_nn neighbours is finished here, with no storage.  One that
//               finds more is appended to the capped list (its place there does not reach the output)
//   cap         one lane per capped voxel, 64 lanes per workgroup: a second walk selects the max_nn smallest
//               (d2, key) through a per-lane list in LDS, a third accumulates those in key order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "normals_core.hpp"
#include "voxel.hpp"

namespace mc {

constexpr int kNrmCapBlock = 64;   // lanes per workgroup of the cap kernel: 64 * 64 * (8 + 2) B = 40 KB of LDS

struct NrmArgs {
  NormalsGrid g;
  const uint32_t* vslot;
  int64_t M;
  NormalsQuery q;
  double viewpoint[3];
  int32_t has_viewpoint;
  double* normals;     // (M, 4) nx, ny, nz, curvature; 16-byte aligned
  int32_t* counts;     // (M,) or null
  double* cov;         // (M, 6) or null; 16-byte aligned
  uint32_t* capped;    // M: the voxels the cap applies to
  uint32_t* n_capped;  // [0]
};

__global__ __launch_bounds__(kVoxBlock) void k_nrm_centroids(VoxOut a, double* cent) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  int32_t k[3];
  double out[4];
  int64_t n;
  vox_finalise_one(a, v, k, out, &n);
  double2* o = reinterpret_cast<double2*>(cent + kNormalsCent * v);
  o[0] = make_double2(out[0], out[1]);
  o[1] = make_double2(out[2], 0.0);
}

__device__ __forceinline__ void nrm_store(const NrmArgs& a, int64_t v, const NormalsMoments& m, int32_t n,
                                          const double ci[3]) {
  double C[6], out[4];
  normals_covariance(m, n, C);
  normals_finish(C, n, ci, a.has_viewpoint != 0, a.viewpoint[0], a.viewpoint[1], a.viewpoint[2], out);
  double2* o = reinterpret_cast<double2*>(a.normals + 4 * v);
  o[0] = make_double2(out[0], out[1]);
  o[1] = make_double2(out[2], out[3]);
  if (a.counts) a.counts[v] = n;
  if (a.cov) {
    double2* c = reinterpret_cast<double2*>(a.cov + 6 * v);
    c[0] = make_double2(C[0], C[1]);
    c[1] = make_double2(C[2], C[3]);
    c[2] = make_double2(C[4], C[5]);
  }
}

__device__ __forceinline__ void nrm_voxel(const NrmArgs& a, int64_t v, int32_t ki[3], double ci[3]) {
  voxel_unpack(a.g.keys[a.vslot[v]], ki);
  const double* c = a.g.cent + kNormalsCent * v;
  ci[0] = c[0];
  ci[1] = c[1];
  ci[2] = c[2];
}

__global__ __launch_bounds__(kVoxBlock) void k_nrm_window(NrmArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  int32_t ki[3];
  double ci[3];
  nrm_voxel(a, v, ki, ci);
  NormalsMoments m;
  const int32_t found = normals_gather(a.g, ki, ci, a.q, &m);
  if (a.q.max_nn != 0 && found > a.q.max_nn) {
    a.capped[atomicAdd(a.n_capped, 1u)] = (uint32_t)v;   // fewer than M appends: inside the list
    return;
  }
  nrm_store(a, v, m, found, ci);
}

__global__ __launch_bounds__(kNrmCapBlock) void k_nrm_cap(NrmArgs a) {
  __shared__ double list_d2[kNormalsMaxNN * kNrmCapBlock];
  __shared__ uint16_t list_ix[kNormalsMaxNN * kNrmCapBlock];
  const int64_t i = (int64_t)blockIdx.x * kNrmCapBlock + threadIdx.x;
  if (i >= (int64_t)*a.n_capped) return;
  const int64_t v = a.capped[i];
  int32_t ki[3];
  double ci[3];
  nrm_voxel(a, v, ki, ci);
  // entry e of lane l at [e * 64 + l]: max_nn <= kNormalsMaxNN entries, so inside both arrays
  double last_d2;
  int32_t last_ix;
  normals_select(a.g, ki, ci, a.q, list_d2 + threadIdx.x, list_ix + threadIdx.x, kNrmCapBlock, &last_d2, &last_ix);
  NormalsMoments m;
  const int32_t kept = normals_gather_capped(a.g, ki, ci, a.q, last_d2, last_ix, &m);
  nrm_store(a, v, m, kept, ci);
}

}  // namespace mc
