// block.hpp — what the scanners (scan.hpp, raymarch.hpp) share with kernels.hpp and with each other:
// the workgroup size, the float64 row transform and the scene's column layout.  Defines no __global__
// function, so any number of translation units may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mc {

constexpr int kBlock = 256;                    // 4 waves of 64

// float64 rows, the reference's own arrays bit for bit:
// R p + t (LMC:775: (R @ p.T).T + t) the way numpy's matmul accumulates it: per output an ascending
// FMA chain over k, fma(R[i][2], z, fma(R[i][1], y, R[i][0] * x)), then + t[i] rounded on its own
// (numpy's dgemm, measured on the reference's box: tools/fma_order.py).  P = {R row-major | t}; with
// the host's scipy-faithful R (rot.cpp) the result equals the reference's float64 value exactly.
// A one-point frame is a matrix-vector product for numpy (its dgemv), which accumulates
// fma(R[i][2], z, fma(R[i][0], x, R[i][1] * y)) instead (tools/fma_order.py, single-row cases): `single`.
__device__ __forceinline__ void frame_apply(const double* __restrict__ P, double x, double y, double z, double& ox,
                                            double& oy, double& oz, bool single = false) {
#pragma clang fp contract(off)
  if (single) {
    ox = __builtin_fma(P[2], z, __builtin_fma(P[0], x, P[1] * y)) + P[9];
    oy = __builtin_fma(P[5], z, __builtin_fma(P[3], x, P[4] * y)) + P[10];
    oz = __builtin_fma(P[8], z, __builtin_fma(P[6], x, P[7] * y)) + P[11];
  } else {
    ox = __builtin_fma(P[2], z, __builtin_fma(P[1], y, P[0] * x)) + P[9];
    oy = __builtin_fma(P[5], z, __builtin_fma(P[4], y, P[3] * x)) + P[10];
    oz = __builtin_fma(P[8], z, __builtin_fma(P[7], y, P[6] * x)) + P[11];
  }
}

// the scene columns x, y, z, intensity (float64) in one allocation of scene_words(E) doubles
inline size_t scene_words(int64_t E) { return 4 * (size_t)E; }
struct SceneCols {
  const double* x; const double* y; const double* z; const double* w;
};
__host__ __device__ inline SceneCols scene_cols(const double* env, int64_t E) {
  return SceneCols{env, env + E, env + 2 * E, env + 3 * E};
}

}  // namespace mc
