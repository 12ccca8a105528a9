// raymarch.hpp — gfx950 kernels for LiDARSimulator.simulate_scan (CSIM:1011-1055), the ray-march
// scanner that produces Path B's input frames: every ray of every frame against a static scene of
// point objects, all frames in one count launch and one emit launch.
//
// The reference marches each ray in steps d_k = np.arange(range_min, range_max, 0.1)[k] and, at each
// sample c = origin + direction * d_k, takes np.linalg.norm(obj[:, :3] - c, axis=1) over every scene
// object (_raycast, CSIM:1108-1146).  The first step with a point closer than 0.1 decides the hit:
// the first object in list order that has such a point, within it the closest point (lowest index on
// ties).  That is the minimum of the key (k, object, distance, point index) over all (step, point)
// pairs with distance < 0.1, and a point can only be that close to sample k when it lies inside the
// ray's 0.1 tube and its along-ray coordinate s is within 0.1 of d_k.  So per (ray, point) the
// kernel runs a conservative tube test (ray_tube: perp^2 <= (0.1 (1 + 1e-5))^2, s inside the marched
// range +- 0.2) and only for the rare candidate the reference's own float64 predicate (ray_exact:
// separate multiply and add for the sample, sqrt((dx dx + dy dy) + dz dz) < 0.1, no contraction) at
// the six steps around (s - range_min) / 0.1.  The work per pair does not depend on the step count.
//
// k_ray_count: a workgroup owns kBlock consecutive rays of the call's frames (one ray per lane:
// its frame's origin, its world direction and best key in registers) and one chunk of the scene, streamed through LDS tiles of
// kRayTile points that every lane reads at the same address (a broadcast).  Its per-chunk best keys
// go to a scratch array; k_ray_merge takes their minimum in key order, so the result depends neither
// on the chunking nor on the grid.  k_ray_emit compacts the hits of a frame in ray order (ballot
// ranks, as k_scan_emit), forms the sensor-frame point R_inv (hit - position) in numpy's one-row
// order, adds the host-drawn noise and writes float64 rows or a float32 batch.
//
// The section between the CORE markers is plain C++ behind RM_HD: tests/host/raymarch_host.cpp
// compiles the same text for the CPU under the sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

// RAYMARCH_CORE_BEGIN
#if defined(__HIPCC__)
#define RM_HD __host__ __device__
#define RM_NOINLINE __attribute__((noinline))
#else
#define RM_HD
#define RM_NOINLINE
#endif

namespace mcray {

// (step << 32 | object), the distance's bits (non-negative doubles order as their bits), scene index
struct RayKey {
  uint64_t ko, dist, idx;
};
constexpr uint64_t kRayMiss = ~0ull;

RM_HD inline bool ray_key_less(const RayKey& a, const RayKey& b) {
  if (a.ko != b.ko) return a.ko < b.ko;
  if (a.dist != b.dist) return a.dist < b.dist;
  return a.idx < b.idx;
}

struct Ray {
  double ox, oy, oz;   // sensor position
  double wx, wy, wz;   // world direction R @ direction
};

// the march of one call: steps[k] = np.arange(range_min, range_max, step)[k], uploaded from numpy
struct RayMarch {
  double range_min;    // steps[0]
  double step;         // 0.1: the step size and the hit radius (CSIM:1118, 1131)
  double s_lo, s_hi;   // along-ray coordinates a close point can have: the marched range +- 2 steps
  double tube2;        // (step (1 + 1e-5))^2
  int32_t K;           // number of steps
};

RM_HD inline RayMarch make_ray_march(const double* steps, int32_t K, double step) {
  RayMarch m;
  m.K = K;
  m.step = step;
  m.range_min = K > 0 ? steps[0] : 0.0;
  m.s_lo = m.range_min - 2.0 * step;
  m.s_hi = (K > 0 ? steps[K - 1] : 0.0) + 2.0 * step;
  const double t = step * (1.0 + 1e-5);
  m.tube2 = t * t;
  return m;
}

// R @ d for one vector, numpy's one-row (matrix-vector) order for a 3x3:
// fma(a2, x2, fma(a0, x0, a1 * x1)).  Forms the world direction (CSIM:1105-1106) and the
// sensor-frame point (CSIM:1170-1171).
RM_HD inline void ray_rotate(const double* A, double x, double y, double z, double& ox, double& oy, double& oz) {
#pragma clang fp contract(off)
  ox = __builtin_fma(A[2], z, __builtin_fma(A[0], x, A[1] * y));
  oy = __builtin_fma(A[5], z, __builtin_fma(A[3], x, A[4] * y));
  oz = __builtin_fma(A[8], z, __builtin_fma(A[6], x, A[7] * y));
}

// current_point = origin + direction * distance (CSIM:1122): a multiply, then an add
RM_HD inline void ray_sample(const Ray& r, double d, double& cx, double& cy, double& cz) {
#pragma clang fp contract(off)
  const double mx = r.wx * d, my = r.wy * d, mz = r.wz * d;
  cx = r.ox + mx;
  cy = r.oy + my;
  cz = r.oz + mz;
}

// Conservative filter: false only for points that cannot be within `step` of any sample of the ray
// (ray_tube) up to along-ray coordinate s_max (ray_in_range).  Rounding here (contraction allowed) is ~1e-11 at 260 m, far inside the
// 1e-5 relative widening of the tube.
RM_HD inline bool ray_tube(const Ray& r, const RayMarch& m, double px, double py, double pz, double& s) {
  const double vx = px - r.ox, vy = py - r.oy, vz = pz - r.oz;
  s = vx * r.wx + vy * r.wy + vz * r.wz;
  const double v2 = vx * vx + vy * vy + vz * vz;
  const double perp2 = v2 - s * s;
  return perp2 <= m.tube2;
}
// ... and, for the few points inside the tube, the along-ray range
RM_HD inline bool ray_in_range(const RayMarch& m, double s_max, double s) { return s >= m.s_lo && s <= s_max; }

// The reference's predicate (CSIM:1122, 1130-1131) for a tube candidate at the steps around s: the
// first step with distance < step gives this point's key; `best` keeps the minimum.
RM_HD RM_NOINLINE inline void ray_exact(const Ray& r, const RayMarch& m, const double* steps, double px, double py,
                                        double pz, double s, uint32_t obj, uint64_t idx, RayKey& best) {
#pragma clang fp contract(off)
  double q = floor((s - m.range_min) / m.step);
  q = q < -4.0 ? -4.0 : (q > (double)m.K + 4.0 ? (double)m.K + 4.0 : q);
  const int32_t k0 = (int32_t)q;
  const int32_t ka = k0 - 2 < 0 ? 0 : k0 - 2;
  const int32_t kb = k0 + 3 > m.K - 1 ? m.K - 1 : k0 + 3;
  for (int32_t k = ka; k <= kb; ++k) {
    double cx, cy, cz;
    ray_sample(r, steps[k], cx, cy, cz);
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    const double sq = (dx * dx + dy * dy) + dz * dz;   // np.add.reduce over the 3 squares
    const double dist = sqrt(sq);
    if (dist < m.step) {
      RayKey key;
      key.ko = ((uint64_t)(uint32_t)k << 32) | obj;
      __builtin_memcpy(&key.dist, &dist, 8);
      key.idx = idx;
      if (ray_key_less(key, best)) best = key;
      return;   // this point's later steps have larger keys
    }
  }
}

// after a hit at step k nothing with s > steps[k] + 2 step can beat it (a point close at a step
// <= k has s < steps[k] + step)
RM_HD inline double ray_s_max(const RayMarch& m, const double* steps, const RayKey& best) {
  return best.ko == kRayMiss ? m.s_hi : steps[best.ko >> 32] + 2.0 * m.step;
}

}  // namespace mcray
// RAYMARCH_CORE_END

#if defined(__HIPCC__)
#include "block.hpp"
#include "layout.hpp"

namespace mc {
using namespace mcray;

constexpr int kRayTile = 512;   // scene points per LDS tile: 3 columns x 512 x 8 B = 12 KB

// the discrete result of one ray: the hit's step, object (position in the caller's list) and scene
// index, or -1 / -1 / -1
struct RayHit {
  int32_t step, obj;
  int64_t idx;
};

struct RayCountArgs {
  const double* scene; int64_t E;   // columns x, y, z, intensity (block.hpp scene_cols)
  const int32_t* obj;               // object of every scene point
  const double* frame;              // per frame: origin (3), R (9)
  const double* dirs; int32_t n_rays;   // sensor-frame unit directions (n_rays, 3)
  const double* steps; RayMarch m;
  int32_t F, n_groups, n_chunks;    // grid = n_groups * n_chunks, n_groups = ceil(F * n_rays / kBlock)
  int64_t chunk_pts;                // scene points per chunk, a multiple of kRayTile
  RayKey* partial;                  // [F][n_rays][n_chunks]
};

__device__ __forceinline__ Ray ray_of(const double* __restrict__ frame, const double* __restrict__ dirs, int32_t f,
                                      int32_t ray) {
  const double* P = frame + 12 * (int64_t)f;
  const double* d = dirs + 3 * (int64_t)ray;
  Ray r;
  r.ox = P[0]; r.oy = P[1]; r.oz = P[2];
  ray_rotate(P + 3, d[0], d[1], d[2], r.wx, r.wy, r.wz);
  return r;
}

__global__ __launch_bounds__(kBlock) void k_ray_count(const RayCountArgs a) {
  __shared__ double s_x[kRayTile], s_y[kRayTile], s_z[kRayTile];
  const int32_t c = blockIdx.x % a.n_chunks;
  const int64_t gr = (int64_t)(blockIdx.x / a.n_chunks) * kBlock + threadIdx.x;   // ray among all frames' rays
  const bool active = gr < (int64_t)a.F * a.n_rays;
  const int32_t f = active ? (int32_t)(gr / a.n_rays) : 0, ray = active ? (int32_t)(gr % a.n_rays) : 0;
  const Ray r = ray_of(a.frame, a.dirs, f, ray);
  const SceneCols sc = scene_cols(a.scene, a.E);
  RayKey best{kRayMiss, kRayMiss, kRayMiss};
  double s_max = a.m.s_hi;
  const int64_t e0 = (int64_t)c * a.chunk_pts;
  const int64_t e1 = e0 + a.chunk_pts < a.E ? e0 + a.chunk_pts : a.E;
  for (int64_t t0 = e0; t0 < e1; t0 += kRayTile) {
    const int n = e1 - t0 < kRayTile ? (int)(e1 - t0) : kRayTile;
    __syncthreads();   // the previous tile has been read by every wave
    for (int i = threadIdx.x; i < n; i += kBlock) {
      s_x[i] = sc.x[t0 + i]; s_y[i] = sc.y[t0 + i]; s_z[i] = sc.z[t0 + i];
    }
    __syncthreads();
    if (active) {
      // One point per branch, rolled by 4: grouping several points' tests under one branch, or inlining
      // ray_exact, raised the loop's registers from 96 to 128-180 and ran 7-25 % slower.
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        const double px = s_x[j], py = s_y[j], pz = s_z[j];   // one address per wave: broadcast reads
        double s;
        if (ray_tube(r, a.m, px, py, pz, s)) {
          if (ray_in_range(a.m, s_max, s)) {
            ray_exact(r, a.m, a.steps, px, py, pz, s, (uint32_t)a.obj[t0 + j], (uint64_t)(t0 + j), best);
            s_max = ray_s_max(a.m, a.steps, best);
          }
        }
      }
    }
  }
  if (active) a.partial[gr * a.n_chunks + c] = best;
}

// minimum of a ray's per-chunk keys, in key order -> the ray's RayHit
__global__ __launch_bounds__(kBlock) void k_ray_merge(const RayKey* __restrict__ partial, int64_t n, int32_t n_chunks,
                                                      RayHit* __restrict__ hit) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  RayKey best{kRayMiss, kRayMiss, kRayMiss};
  for (int32_t c = 0; c < n_chunks; ++c) {
    const RayKey k = partial[i * n_chunks + c];
    if (ray_key_less(k, best)) best = k;
  }
  RayHit h{-1, -1, -1};
  if (best.ko != kRayMiss) {
    h.step = (int32_t)(best.ko >> 32);
    h.obj = (int32_t)(uint32_t)best.ko;
    h.idx = (int64_t)best.idx;
  }
  hit[i] = h;
}

struct RayEmitArgs {
  const double* scene; int64_t E;
  const double* frame;              // origin (3), R (9) per frame, as the count used them
  const double* rinv;               // R_inv (9) per frame (CSIM:1170)
  const double* dirs; int32_t n_rays;
  const double* steps;
  const RayHit* hit;                // [F][n_rays]
  const double* noise;              // (H, 4): x, y, z, intensity noise per hit in frame / ray order, or nullptr
  const int64_t* poff; const int64_t* doff;   // the output's frame offsets (poff: batch only)
  double* rows;                     // ROWS: (H, 5) x, y, z, intensity, ray index
  float* cols; int32_t C;           // batch: blocked columns (x | y | z | intensity [| t_ns])
  int32_t* pcd_len;                 // batch, MC_BATCH_WITH_PCD_LEN: per-block text bytes (zeroed), or nullptr
};

// one workgroup per frame: hits compacted in ray order
template <bool ROWS>
__global__ __launch_bounds__(kBlock) void k_ray_emit(const RayEmitArgs a) {
  __shared__ int s_cnt[kBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int32_t f = blockIdx.x;
  const SceneCols sc = scene_cols(a.scene, a.E);
  const double* P = a.frame + 12 * (int64_t)f;
  const double* Ri = a.rinv + 9 * (int64_t)f;
  const int64_t doff = a.doff[f], poff = ROWS ? 0 : a.poff[f];
  int64_t base = 0;
  for (int32_t r0 = 0; r0 < a.n_rays; r0 += kBlock) {
    const int32_t ray = r0 + threadIdx.x;
    RayHit h{-1, -1, -1};
    if (ray < a.n_rays) h = a.hit[(int64_t)f * a.n_rays + ray];
    const bool is_hit = h.step >= 0;
    const unsigned long long mask = __ballot(is_hit);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wid] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const int n = s_cnt[w];
      before += w < wid ? n : 0;
      total += n;
    }
    if (is_hit) {
#pragma clang fp contract(off)
      const int64_t o = base + before + rank;   // index among the frame's hits
      const Ray r = ray_of(a.frame, a.dirs, f, ray);
      double cx, cy, cz;
      ray_sample(r, a.steps[h.step], cx, cy, cz);             // hit_point = current_point (CSIM:1139)
      const double tx = cx - P[0], ty = cy - P[1], tz = cz - P[2];   // CSIM:1152
      double lx, ly, lz;
      ray_rotate(Ri, tx, ty, tz, lx, ly, lz);                  // CSIM:1171
      double w = sc.w[h.idx];
      if (a.noise) {                                           // CSIM:1038-1039: one rounding each
        const double* q = a.noise + 4 * (doff + o);
        lx = lx + q[0]; ly = ly + q[1]; lz = lz + q[2];
        w = w + q[3];
      }
      w = w < 0.0 ? 0.0 : (w > 255.0 ? 255.0 : w);             // np.clip(intensity, 0, 255), CSIM:1040
      if constexpr (ROWS) {
        double* q = a.rows + 5 * (doff + o);
        q[0] = lx; q[1] = ly; q[2] = lz; q[3] = w; q[4] = (double)ray;
      } else {
        float* q = a.cols + bidx(a.C, 0, poff + o);
        const float v[4] = {(float)lx, (float)ly, (float)lz, (float)w};
        q[0] = v[0];
        q[kBlkPts] = v[1];
        q[2 * kBlkPts] = v[2];
        q[3 * kBlkPts] = v[3];
        if (a.C == 5) reinterpret_cast<int32_t*>(q)[4 * kBlkPts] = ray * 1000;   // CSIM:1048, ns since the frame start
        if (a.pcd_len) {   // this line's text bytes (layout.hpp PcdCount), one atomic per point
          PcdCount pc;
          pc.add2(true, v[0], v[1]);
          pc.add2(true, v[2], v[3]);
          atomicAdd(a.pcd_len + ((poff + o) >> 8), pc.lane_bytes() + (pc.lane_slow() ? kPcdSlowValue : 0));
        }
      }
    }
    base += total;
    __syncthreads();   // s_cnt is rewritten by the next ray group
  }
}

}  // namespace mc
#endif  // __HIPCC__
