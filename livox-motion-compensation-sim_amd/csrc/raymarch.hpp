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
// The per-pair core (ray_tube, ray_exact, ray_key_less, ...) is raymarch_core.hpp: plain C++ that
// tests/host/raymarch_host.cpp compiles for the CPU under the sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "raymarch_core.hpp"

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
