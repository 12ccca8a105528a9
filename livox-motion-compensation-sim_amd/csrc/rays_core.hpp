// rays_core.hpp — the scalar core of the voxel cloud's ray walk (rays.hpp), on plain values so the same text compiles
// for the device and for the host (tests/host/rays_host.cpp includes it; built with g++ -ffp-contract=off).  A core
// header (DESIGN.md "Core headers"); needs no stand-in.  No HIP include.
//
// The ray of a source point runs from the sensor position s to the point e, both in the cloud's frame.  Its walk
// through the cloud's grid is a function of s, e, h and o alone (include/mcdeskew.h "rays through the voxel cloud").
// Every line of floating-point arithmetic is ONE IEEE float64 operation, never contracted:
//   grid     per axis a, the filter's own lines (voxel_core.hpp) with the cloud's h and origin o:
//              as = s - o     gs = as / h     ks = floor(gs)          ae = e - o     ge = ae / h     ke = floor(ge)
//            so ke is exactly the cell an insert puts the point in
//   skipped  a ray whose s or e voxel_quantise refuses (intensity taken as 0.0: a coordinate or g that is not finite, a
//            key outside [-2^20, 2^20)), or whose walk has more than max_steps steps: it counts nowhere
//   walk     d_a = ge_a - gs_a     dir_a = +1 when ke_a > ks_a, -1 when ke_a < ks_a, else 0     n_a = |ke_a - ks_a|
//            steps = n_x + n_y + n_z: the walk has exactly that many transitions and always ends in ke
//            the j-th crossing on axis a (j = 0 .. n_a - 1):
//              b = double(ks_a + j dir_a + (dir_a > 0 ? 1 : 0))     u = b - gs_a     t_a(j) = u / d_a
//            from j alone, never accumulated; an axis with its n_a crossings done has t_a = +inf.  Each transition
//            takes the axis of smallest current t_a, ties to the lowest axis, and moves one cell along it.  No
//            comparison sees a NaN: n_a > 0 implies d_a != 0
//   cells    position 0 is ks, position `steps` is ke, and the cells of one walk are distinct
//            ended   the voxel of ke, when the cloud holds one
//            passed  the voxels of positions 0 .. steps - 1 - guard, where the cloud holds them (a guard larger than
//                    the walk leaves none); `through` is their number
#pragma once
#include <math.h>
#include <stdint.h>

#include "normals_core.hpp"

namespace mc {

constexpr int32_t kRaysMaxGuard = 255;
constexpr int32_t kRaysMaxSteps = 1 << 22;   // three axes of fewer than 2^21 crossings each stay below it
constexpr int32_t kRaysSkipped = -1;         // `through` of a ray that is not walked

// the live voxel build as the walk reads it: the key table and the voxel of each slot (g.cent is not read), the
// number of voxels (0: there is no table) and the grid
struct RaysGrid {
  NormalsGrid g;
  int64_t M;
  double h, o[3];
};

// a walk in progress: the cell it stands in, what is left of it, and the crossing parameter of every axis
struct RaysWalk {
  double gs[3], d[3], t[3];
  int32_t k[3], ke[3];
  int32_t dir[3], left[3];   // left: the crossings the axis has still to make
  int32_t steps;             // n_x + n_y + n_z
};

// the grid lines of one end of a ray -> false: voxel_quantise refuses it
MC_CORE_HD bool rays_cell(double h, const double o[3], const double v[3], double g[3], int32_t k[3]) {
  MC_CORE_NO_CONTRACT
  const VoxelPoint q = voxel_quantise(v, 0.0, h, o);
  for (int a = 0; a < 3; ++a) {
    const double d = v[a] - o[a];
    g[a] = d / h;
    k[a] = q.k[a];
  }
  return !q.bad;
}

// t_a of an axis's next crossing, from the cell the walk stands in on that axis: k = ks_a + j dir_a, `left` = n_a - j
MC_CORE_HD double rays_crossing(int32_t k, int32_t dir, int32_t left, double gs, double d) {
  MC_CORE_NO_CONTRACT
  if (left == 0) return (double)INFINITY;
  const double b = (double)(k + (dir > 0 ? 1 : 0));
  const double u = b - gs;
  return u / d;
}

// the walk of the ray s -> e on the grid (h, o) -> false: skipped
MC_CORE_HD bool rays_begin(double h, const double o[3], const double s[3], const double e[3], int32_t max_steps, RaysWalk* w) {
  MC_CORE_NO_CONTRACT
  double ge[3];
  const bool s_ok = rays_cell(h, o, s, w->gs, w->k);
  const bool e_ok = rays_cell(h, o, e, ge, w->ke);
  if (!s_ok || !e_ok) return false;
  int64_t steps = 0;
  for (int a = 0; a < 3; ++a) {
    w->d[a] = ge[a] - w->gs[a];
    w->dir[a] = w->ke[a] > w->k[a] ? 1 : (w->ke[a] < w->k[a] ? -1 : 0);
    w->left[a] = w->dir[a] > 0 ? w->ke[a] - w->k[a] : w->k[a] - w->ke[a];   // < 2^21
    steps += w->left[a];
  }
  if (steps > (int64_t)max_steps) return false;
  w->steps = (int32_t)steps;
  for (int a = 0; a < 3; ++a) w->t[a] = rays_crossing(w->k[a], w->dir[a], w->left[a], w->gs[a], w->d[a]);
  return true;
}

// One transition (the walk has some left): the axis of smallest t, ties to the lowest; only its t changes.  The axis
// is a value, not an index: its fields are picked and put back by selects under constant indices, so the state stays
// in registers on the device, and the one division serves whichever axis each lane moves on
MC_CORE_HD void rays_step(RaysWalk* w) {
  double best = w->t[0];
  int a = 0;
  if (w->t[1] < best) { a = 1; best = w->t[1]; }
  if (w->t[2] < best) { a = 2; best = w->t[2]; }
  // every field is read before the axis is looked at and written whichever axis moves: no access depends on `a`
  const int32_t k3[3] = {w->k[0], w->k[1], w->k[2]}, dir3[3] = {w->dir[0], w->dir[1], w->dir[2]};
  const int32_t left3[3] = {w->left[0], w->left[1], w->left[2]};
  const double gs3[3] = {w->gs[0], w->gs[1], w->gs[2]}, d3[3] = {w->d[0], w->d[1], w->d[2]}, t3[3] = {w->t[0], w->t[1], w->t[2]};
  const int32_t dir = a == 1 ? dir3[1] : (a == 2 ? dir3[2] : dir3[0]);
  const int32_t k = (a == 1 ? k3[1] : (a == 2 ? k3[2] : k3[0])) + dir;
  const int32_t left = (a == 1 ? left3[1] : (a == 2 ? left3[2] : left3[0])) - 1;
  const double gs = a == 1 ? gs3[1] : (a == 2 ? gs3[2] : gs3[0]);
  const double d = a == 1 ? d3[1] : (a == 2 ? d3[2] : d3[0]);
  const double t = rays_crossing(k, dir, left, gs, d);
  MC_CORE_UNROLL
  for (int c = 0; c < 3; ++c) {
    w->k[c] = c == a ? k : k3[c];
    w->left[c] = c == a ? left : left3[c];
    w->t[c] = c == a ? t : t3[c];
  }
}

// the voxel of a cell of the walk (its keys lie between two accepted cells: inside the key range)
MC_CORE_HD bool rays_voxel(const RaysGrid& G, const int32_t k[3], uint32_t* v) {
  return G.M > 0 && normals_find(G.g, voxel_pack(k), v);
}

// The ray s -> e through the cloud: fn_passed(v) for the voxel of every position 0 .. steps - 1 - guard that the cloud
// holds, in walk order, then fn_ended(v) for the voxel of ke when it holds one.  -> `through`, the voxels handed to
// fn_passed, or kRaysSkipped with nothing called; *steps: the transitions walked (0 for a skipped ray)
template <typename FnPassed, typename FnEnded>
MC_CORE_HD int32_t rays_walk(const RaysGrid& G, const double s[3], const double e[3], int32_t guard, int32_t max_steps,
                             FnPassed&& fn_passed, FnEnded&& fn_ended, int32_t* steps) {
  RaysWalk w;
  *steps = 0;
  if (!rays_begin(G.h, G.o, s, e, max_steps, &w)) return kRaysSkipped;
  *steps = w.steps;
  const int32_t counted = w.steps - guard;   // the positions below it count as passed
  int32_t through = 0;
  uint32_t v;
  for (int32_t at = 0; at < w.steps; ++at) {
    if (at < counted && rays_voxel(G, w.k, &v)) {
      fn_passed(v);
      ++through;
    }
    rays_step(&w);
  }
  if (rays_voxel(G, w.k, &v)) fn_ended(v);
  return through;
}

}  // namespace mc
