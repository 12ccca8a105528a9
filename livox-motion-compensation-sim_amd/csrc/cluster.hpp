// cluster.hpp — the kernels of the voxel cloud's density clustering (host side in voxel.hip; scalar core in
// cluster_core.hpp).  They read the live voxel build as the normals do (its key table, vid, vslot, cnt and the
// centroids by voxel id) and keep one `parent` word and one label per voxel.
//
// Five phases, one lane per voxel:
//   density   the window walk counts the neighbours (or sums their points); parent[v] = v for a core voxel,
//             kClusterNone otherwise
//   union     a core voxel walks the half of its window after the centre and unites itself with every core
//             neighbour there: a lock-free union-find (cluster_core.hpp).  Inside
//             this launch `parent` is read with relaxed agent-scope atomic loads only (per-XCD L2s and per-CU
//             L1s are not coherent inside a launch; a stale value is harmless, the compare-and-swap decides),
//             linked with atomicCAS and shortened with atomicMin.  No lane waits for another.
//   label     a new launch: a core voxel takes its root, another the root of its best core neighbour or noise
//   number    the roots (label[v] == v) flagged and scanned by voxel id (vox_block_scan, k_vox_scan), the root's
//             number left in its own parent word, then every label rewritten to 0 .. K - 1
//   stats     per cluster, on request: voxels, source points, the cells' bounding box, with integer atomic adds,
//             minima and maxima (order-independent); a wave whose voxels share one cluster adds once
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cluster_core.hpp"
#include "voxel.hpp"

namespace mc {

// `parent` as the union phase reads and writes it
struct ClusterDevMem {
  uint32_t* p;
  __device__ __forceinline__ uint32_t load(uint32_t i) const {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expected, uint32_t value) {
    return atomicCAS(p + i, expected, value);
  }
  __device__ __forceinline__ void lower(uint32_t i, uint32_t value) { (void)atomicMin(p + i, value); }
};

struct ClusterArgs {
  NormalsGrid g;
  const uint32_t* vslot;
  const uint32_t* cnt;      // source points by voxel id
  int64_t M;
  NormalsQuery q;
  int32_t min_points;
  int32_t weighted;
  uint32_t* parent;         // M
  uint32_t* label;          // M: the root's id, then the cluster's number (kClusterNone: noise)
  uint32_t* chunk;          // ceil(M / kVoxBlock): roots per workgroup, then their exclusive scan
  int32_t* labels_out;      // (M,)
  int32_t* density_out;     // (M,) or null
};

__device__ __forceinline__ void cluster_voxel(const ClusterArgs& a, int64_t v, int32_t ki[3], double ci[3]) {
  voxel_unpack(a.g.keys[a.vslot[v]], ki);
  const double* c = a.g.cent + kNormalsCent * v;
  ci[0] = c[0];
  ci[1] = c[1];
  ci[2] = c[2];
}

__global__ __launch_bounds__(kVoxBlock) void k_cl_density(ClusterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  int32_t ki[3];
  double ci[3];
  cluster_voxel(a, v, ki, ci);
  const int32_t density = cluster_density(a.g, ki, ci, a.q, a.weighted ? a.cnt : nullptr);
  a.parent[v] = cluster_seed((uint32_t)v, density, a.min_points);
  if (a.density_out) a.density_out[v] = density;
}

__global__ __launch_bounds__(kVoxBlock) void k_cl_union(ClusterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  ClusterDevMem m = {a.parent};
  if (m.load((uint32_t)v) == kClusterNone) return;
  int32_t ki[3];
  double ci[3];
  cluster_voxel(a, v, ki, ci);
  cluster_union_voxel(a.g, ki, ci, a.q, m, (uint32_t)v);
}

__global__ __launch_bounds__(kVoxBlock) void k_cl_label(ClusterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  ClusterDevMem m = {a.parent};
  int32_t ki[3];
  double ci[3];
  cluster_voxel(a, v, ki, ci);
  a.label[v] = cluster_root_voxel(a.g, ki, ci, a.q, m, (uint32_t)v);
}

// the roots of the workgroup's voxels counted (every thread reaches the scan)
__global__ __launch_bounds__(kVoxBlock) void k_cl_flag(ClusterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  const uint32_t root = v < a.M && a.label[v] == (uint32_t)v;
  uint32_t excl;
  const uint32_t total = vox_block_scan(root, &excl);
  if (threadIdx.x == 0) a.chunk[blockIdx.x] = total;
}

// a root's number into its parent word (the trees are not needed any more)
__global__ __launch_bounds__(kVoxBlock) void k_cl_rank(ClusterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  const uint32_t root = v < a.M && a.label[v] == (uint32_t)v;
  uint32_t excl;
  vox_block_scan(root, &excl);
  if (root) a.parent[v] = a.chunk[blockIdx.x] + excl;
}

__global__ __launch_bounds__(kVoxBlock) void k_cl_number(ClusterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  const uint32_t root = a.label[v];
  const uint32_t number = root == kClusterNone ? kClusterNone : a.parent[root];   // root < M: a voxel's id
  a.label[v] = number;
  a.labels_out[v] = root == kClusterNone ? kClusterNoise : (int32_t)number;
}

struct ClusterStatsArgs {
  const unsigned long long* keys;
  const uint32_t* vslot;
  const uint32_t* cnt;
  const uint32_t* label;    // the cluster's number (kClusterNone: noise)
  int64_t M;
  int32_t* voxels;          // (K,) or null; zeroed
  long long* points;        // (K,) or null; zeroed
  int32_t* cell_min;        // (K, 3) or null; every word above any key
  int32_t* cell_max;        // (K, 3) or null; every word below any key
};

__device__ __forceinline__ void cluster_stats_add(const ClusterStatsArgs& a, uint32_t c, int32_t voxels, long long points,
                                                  const int32_t lo[3], const int32_t hi[3]) {
  if (a.voxels) (void)__hip_atomic_fetch_add(a.voxels + c, voxels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (a.points) (void)__hip_atomic_fetch_add(a.points + c, points, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (a.cell_min) (void)atomicMin(a.cell_min + 3 * (int64_t)c + k, lo[k]);
    if (a.cell_max) (void)atomicMax(a.cell_max + 3 * (int64_t)c + k, hi[k]);
  }
}

__global__ __launch_bounds__(kVoxBlock) void k_cl_stats(ClusterStatsArgs a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  uint32_t c = kClusterNone;
  int32_t k[3] = {0, 0, 0};
  long long points = 0;
  if (v < a.M) {
    c = a.label[v];
    if (c != kClusterNone) {
      voxel_unpack(a.keys[a.vslot[v]], k);
      points = a.cnt[v];
    }
  }
  // the wave's clustered voxels in one cluster: one lane adds the wave's sums (a wave that holds two clusters
  // falls back to its lanes' own atomics: DESIGN.md §8 has what that costs).  Integer sums, minima and maxima: the same result either way.
  const unsigned long long in = __ballot(c != kClusterNone);
  if (in == 0) return;   // wave-uniform
  const uint32_t first = (uint32_t)__shfl((int)c, __ffsll((long long)in) - 1, 64);
  if (__all(c == kClusterNone || c == first)) {
    const bool on = c != kClusterNone;
    int32_t voxels = on ? 1 : 0;
    int32_t lo[3], hi[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      lo[j] = on ? k[j] : kVoxelKeyEnd;
      hi[j] = on ? k[j] : kVoxelKeyMin - 1;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      voxels += __shfl_xor(voxels, d, 64);
      points += __shfl_xor(points, d, 64);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        lo[j] = min(lo[j], __shfl_xor(lo[j], d, 64));
        hi[j] = max(hi[j], __shfl_xor(hi[j], d, 64));
      }
    }
    if ((threadIdx.x & 63) == 0) cluster_stats_add(a, first, voxels, points, lo, hi);
    return;
  }
  if (c != kClusterNone) cluster_stats_add(a, c, 1, points, k, k);
}

}  // namespace mc
