// rays.hpp — the kernel of the ray walk through the voxel cloud (host side in voxel.hip; scalar core in rays_core.hpp).
// It reads the live voxel build through the key table and vid alone (no centroids) and changes nothing of it.
//
//   clear   passed and ended zeroed, and the call's two counters (memsets on the stream)
//   walk    one ray per lane: the sensor position to the source point, rays_walk of the core.  Every occupied cell a
//           ray passes adds 1 to passed[v], the occupied cell it ends in adds 1 to ended[v]: 32-bit integer atomic
//           adds, fewer than 2^31 of them per word, so the counts do not depend on the order they arrive in.  The
//           ray's `through`, -1 for a skipped ray, by a plain store.  The skipped rays and the transitions walked are
//           summed per wave and added with one 64-bit integer atomic each
//
// The lanes of a batch are its padded slots, as the filter's (VoxSrc; voxel.hpp vox_points): the 64 slots of a wave lie
// in one 256-point block, so the frame, and with it the sensor position, is wave-uniform, and a padding slot is no
// ray.  vox_points itself hands a lane four points and not their frame; the walk wants one ray per lane (the lanes of
// a wave leave the loop when the longest of their walks ends) and the frame's origin, so the slot is read here.
//
// Combining.  The first cells of a frame's rays are the same few voxels around the sensor, and one word takes about
// 88 atomics per microsecond (voxel.hpp).  The lanes that stand at a voxel at the same moment and target the voxel of
// the first of them add once, through their lowest lane, the number of them; the others add 1 each.  One
// readfirstlane, one ballot and a population count per counted voxel; whatever lanes are active together, every ray
// is counted exactly once.  Against one atomic per lane it costs 1 % of a batch's walk or less where no voxel is
// contended and is 1.8 to 4 times faster where the sensor's own cell is occupied (DESIGN.md §8 "Rays through the voxel
// cloud").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rays_core.hpp"
#include "voxel.hpp"

namespace mc {

enum { kRaysMetaSkipped = 0, kRaysMetaSteps = 1, kRaysMeta = 2 };

struct RaysArgs {
  VoxSrc src;               // the batch or the rows (src.h and src.o are not read: the grid is G's)
  int64_t slot0, slots;     // a batch: the source's first padded slot and the number of them (a multiple of 256)
  int64_t first;            // a batch: the source's first point among the batch's dense points
  const double* origins;    // (n_origins, 3) sensor positions in the cloud's frame
  int64_t n_origins;        // 1: for every ray; else one per frame (a batch) or per row
  RaysGrid G;
  int32_t guard, max_steps;
  int* passed;              // (M,)
  int* ended;               // (M,)
  int32_t* through;         // (n,)
  unsigned long long* meta; // kRaysMeta words
};

// +1 to counts[v] for every lane that is here
__device__ __forceinline__ void rays_count(int* counts, uint32_t v) {
  const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  const unsigned long long same = __builtin_amdgcn_ballot_w64(v == lead);
  const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
  if (v != lead) atomicAdd(counts + v, 1);
  else if ((same & below) == 0) atomicAdd(counts + v, (int)__builtin_popcountll(same));
}

template <bool BATCH>
__global__ __launch_bounds__(kVoxBlock) void k_rays_walk(RaysArgs a) {
  const int64_t lane = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  bool ray = false;
  int64_t i = 0, at = 0;   // the ray's place in the source, and its sensor position's row
  double e[3] = {0.0, 0.0, 0.0};
  if (BATCH) {
    if (lane < a.slots) {
      const VoxSrc& s = a.src;
      const int64_t pp = a.slot0 + lane;   // < P
      const int64_t blk0 = (int64_t)__builtin_amdgcn_readfirstlane((int)(pp >> 8)) << 8;
      int32_t lo = 0, hi = s.F - 1;
      while (lo < hi) {   // the first frame whose padded end is beyond the block
        const int32_t mid = (lo + hi) >> 1;
        if (ldu(s.poff + mid + 1) <= blk0) lo = mid + 1;
        else hi = mid;
      }
      const int64_t local = pp - ldu(s.poff + lo);
      if (local < ldu(s.counts + lo)) {
        const float* b = s.cols + bidx(s.C, 0, pp);
        e[0] = (double)b[0];
        e[1] = (double)b[kBlkPts];
        e[2] = (double)b[2 * kBlkPts];
        i = ldu(s.doff + lo) + local - a.first;   // 0 <= i < n: the slot is a point of the source
        at = a.n_origins == 1 ? 0 : lo;
        ray = true;
      }
    }
  } else if (lane < a.src.n) {
    const double* r = a.src.rows + lane * a.src.ld;
    e[0] = r[0];
    e[1] = r[1];
    e[2] = r[2];
    i = lane;
    at = a.n_origins == 1 ? 0 : lane;
    ray = true;
  }
  int32_t steps = 0;
  bool skipped = false;
  if (ray) {
    const double* o = a.origins + 3 * at;
    const double s[3] = {o[0], o[1], o[2]};
    const int32_t through = rays_walk(
        a.G, s, e, a.guard, a.max_steps, [&](uint32_t v) { rays_count(a.passed, v); },   // v < M: a voxel of the table
        [&](uint32_t v) { rays_count(a.ended, v); }, &steps);
    a.through[i] = through;
    skipped = through == kRaysSkipped;
  }
  // every lane of the wave is here again: steps <= 2^22 each, 2^28 per wave
  const uint32_t n_skipped = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(skipped));
  const int wave_steps = wave_sum_dpp(steps);
  if ((threadIdx.x & 63) == 0) {
    if (n_skipped) atomicAdd(a.meta + kRaysMetaSkipped, (unsigned long long)n_skipped);
    if (wave_steps) atomicAdd(a.meta + kRaysMetaSteps, (unsigned long long)wave_steps);
  }
}

}  // namespace mc
