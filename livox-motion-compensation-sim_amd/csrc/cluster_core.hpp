// cluster_core.hpp — the scalar core of the voxel cloud's density clustering (cluster.hpp), on plain values so
// the same text compiles for the device and for the host (tests/host/cluster_host.cpp and cluster_tsan_host.cpp
// include it; built with g++ -ffp-contract=off).  A core header (DESIGN.md "Core headers"); needs no stand-in.
// No HIP include.
//
// DBSCAN over the live voxel build, a function of the voxel set alone (include/mcdeskew.h "density clustering"):
//   neighbours  of voxel i: normals_neighbours_v's set at R = ceil(eps / h), r2 = eps * eps, no cap, i included
//   density     their number, or (weighted) the sum of their source-point counts; core when >= min_points
//   cluster     a connected component of the core voxels under the neighbour relation (which is symmetric:
//               u and -u have the same squares, and the window and the key range are symmetric too)
//   border      a non-core voxel with a core neighbour joins that of the smallest (d2, ix); else noise
// The components come from a lock-free union-find on one 4-byte word per voxel, `parent`:
//   kClusterNone for a voxel that is not core; else the id of an ancestor, parent[x] <= x at all times, so a
//   root (parent[x] == x) is the lowest id of its tree and the final root of a component is its lowest voxel
//   id, whatever order the unions arrived in.
//   The only write that links is cas(hi, hi, lo) with lo < hi; path shortening only lowers a word to a value
//   read from an ancestor (lower = an atomic minimum).  Every loop below moves to a strictly smaller id on each
//   turn: nothing waits for another lane.
// Mem is the memory policy over `parent`: uint32_t load(i), uint32_t cas(i, expected, value) -> the word before,
// void lower(i, value).  A load may be stale (an earlier, higher ancestor): find then returns an ancestor that
// is no root any more, the cas on it fails and hands back the word's true value, from which unite goes on.
#pragma once
#include <stdint.h>

#include "normals_core.hpp"

namespace mc {

constexpr uint32_t kClusterNone = 0xFFFFFFFFu;   // parent: not a core voxel; a root id: noise
constexpr int32_t kClusterNoise = -1;            // the label of noise
constexpr int kClusterPhases = 5;                // density, union, label, number, stats

// the neighbour search of a clustering: the normals' window without a cap
MC_CORE_HD NormalsQuery cluster_query(int32_t R, double eps2) {
  NormalsQuery q;
  q.R = R;
  q.max_nn = 0;
  q.r2 = eps2;
  return q;
}

// the centre's place in the walk: the cells after it are the half of the window a union walks
MC_CORE_HD int32_t cluster_centre(int32_t R) {
  const int32_t W = 2 * R + 1;
  return (R * W + R) * W + R;
}

// the neighbours of the voxel, or with cnt (source points by voxel id) the sum of their points
MC_CORE_HD int32_t cluster_density(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                    const uint32_t* cnt) {
  int32_t density = 0;
  normals_neighbours_v(g, ki, ci, q, [&](int32_t, uint32_t j, const double*, double) {
    density += cnt ? (int32_t)cnt[j] : 1;
  });
  return density;
}

// parent's first value
MC_CORE_HD uint32_t cluster_seed(uint32_t v, int32_t density, int32_t min_points) {
  return density >= min_points ? v : kClusterNone;
}

// an ancestor of core voxel x that was a root when it was read, shortening the path on the way
template <typename Mem>
MC_CORE_HD uint32_t cluster_find(Mem& m, uint32_t x) {
  for (;;) {
    const uint32_t p = m.load(x);
    if (p >= x) return x;          // p == x: a root (p > x cannot be: parent[x] <= x)
    const uint32_t gp = m.load(p);
    if (gp < p) m.lower(x, gp);    // gp is an ancestor of x and below what x holds
    x = p;                         // strictly smaller
  }
}

// one tree out of the trees of core voxels a and b
template <typename Mem>
MC_CORE_HD void cluster_unite(Mem& m, uint32_t a, uint32_t b) {
  for (;;) {
    a = cluster_find(m, a);
    b = cluster_find(m, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b;
    const uint32_t lo = a > b ? b : a;
    const uint32_t was = m.cas(hi, hi, lo);
    if (was == hi) return;
    // hi had been linked already (was < hi): go on from its true parent, a strictly smaller id
    a = was;
    b = lo;
  }
}

// union phase of core voxel v: with every core neighbour in the half of the window after the centre, the only
// half the walk probes (the relation is symmetric: the other half is the neighbours' to unite)
template <typename Mem>
MC_CORE_HD void cluster_union_voxel(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                     Mem& m, uint32_t v) {
  normals_neighbours_v<true>(
      g, ki, ci, q,
      [&](int32_t, uint32_t j, const double*, double) {
        if (m.load(j) != kClusterNone) cluster_unite(m, v, j);
      },
      cluster_centre(q.R) + 1);
}

// label phase of voxel v (no link is made any more): the root of its tree; of a voxel that is not core, the
// root of the core neighbour with the smallest (d2, ix), or kClusterNone for noise
template <typename Mem>
MC_CORE_HD uint32_t cluster_root_voxel(const NormalsGrid& g, const int32_t ki[3], const double ci[3], const NormalsQuery& q,
                                        Mem& m, uint32_t v) {
  if (m.load(v) != kClusterNone) return cluster_find(m, v);
  uint32_t best = kClusterNone;
  double best_d2 = 0.0;
  normals_neighbours_v(g, ki, ci, q, [&](int32_t, uint32_t j, const double*, double d2) {
    // the walk ascends in ix, so the first of equal d2 stays
    if (m.load(j) != kClusterNone && (best == kClusterNone || d2 < best_d2)) {
      best = j;
      best_d2 = d2;
    }
  });
  return best == kClusterNone ? kClusterNone : cluster_find(m, best);
}

}  // namespace mc
