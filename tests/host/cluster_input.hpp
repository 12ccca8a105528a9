// What the two host harnesses of the density clustering (cluster_host.cpp, cluster_tsan_host.cpp) share: the
// input file of tests/test_clusters_cpu.py and the build's key table, made here with the filter's own probe
// sequence (voxel_slot_first / voxel_slot_next), the keys inserted in voxel order, as normals_host.cpp does.
//   in:  h, eps, eps2 (3 f64); M, R, min_points, weighted, log2 of the table size, order, seed (7 i64);
//        keys (M, 3) i32; centroids (M, 3) f64; source points (M,) u32
//   order: 0 the voxels forwards, 1 backwards, 2 in a shuffle seeded by seed
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "cluster_core.hpp"

namespace cluster_input {

using namespace mc;

struct Input {
  int64_t M = 0;
  int32_t min_points = 0;
  bool weighted = false;
  NormalsQuery q;
  NormalsGrid g;
  std::vector<int32_t> keys;
  std::vector<uint32_t> cnt;
  std::vector<uint32_t> order;
  // what g points into
  std::vector<unsigned long long> table;
  std::vector<uint32_t> vid;
  std::vector<double> cent;
};

inline std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> d;
  if (FILE* fp = std::fopen(path, "rb")) {
    uint8_t buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) d.insert(d.end(), buf, buf + k);
    std::fclose(fp);
  }
  return d;
}

// 0, or the exit status of a malformed input
inline int read(const char* path, Input* in) {
  const std::vector<uint8_t> raw = slurp(path);
  constexpr size_t kHead = 24 + 56;
  if (raw.size() < kHead) return 2;
  double par[3];
  int64_t dim[7];
  std::memcpy(par, raw.data(), 24);
  std::memcpy(dim, raw.data() + 24, 56);
  const int64_t M = dim[0];
  const int log2cap = (int)dim[4];
  if (M < 0 || dim[1] < 1 || dim[1] > kNormalsMaxR || dim[2] < 1 || log2cap < 6 || log2cap > 30 ||
      ((int64_t)1 << log2cap) < 2 * M || dim[5] < 0 || dim[5] > 2)
    return 2;
  if (raw.size() != kHead + (size_t)M * (12 + 24 + 4)) return 2;
  in->M = M;
  in->min_points = (int32_t)dim[2];
  in->weighted = dim[3] != 0;
  in->q = cluster_query((int32_t)dim[1], par[2]);
  in->keys.resize((size_t)3 * M);
  in->cnt.resize((size_t)M);
  std::vector<double> c3((size_t)3 * M);
  if (M) {
    std::memcpy(in->keys.data(), raw.data() + kHead, (size_t)12 * M);
    std::memcpy(c3.data(), raw.data() + kHead + (size_t)12 * M, (size_t)24 * M);
    std::memcpy(in->cnt.data(), raw.data() + kHead + (size_t)36 * M, (size_t)4 * M);
  }
  const size_t cap = (size_t)1 << log2cap;
  in->table.assign(cap, kVoxelEmpty);
  in->vid.assign(cap, 0xDEADBEEFu);
  in->cent.assign((size_t)kNormalsCent * M + 1, 0.0);
  in->g.shift = 64 - log2cap;
  in->g.mask = (uint32_t)(cap - 1);
  for (int64_t v = 0; v < M; ++v) {
    const uint64_t key = voxel_pack(&in->keys[3 * v]);
    uint32_t at = voxel_slot_first(key, in->g.shift, in->g.mask);
    while (in->table[at] != kVoxelEmpty) {
      if (in->table[at] == key) return 3;   // one voxel per cell
      at = voxel_slot_next(at, in->g.mask);
    }
    in->table[at] = key;
    in->vid[at] = (uint32_t)v;
    for (int a = 0; a < 3; ++a) in->cent[kNormalsCent * v + a] = c3[3 * v + a];
  }
  in->g.keys = in->table.data();
  in->g.vid = in->vid.data();
  in->g.cent = in->cent.data();
  in->order.resize((size_t)M);
  std::iota(in->order.begin(), in->order.end(), 0u);
  if (dim[5] == 1) std::reverse(in->order.begin(), in->order.end());
  if (dim[5] == 2) {
    std::mt19937_64 rng((uint64_t)dim[6]);
    for (size_t i = in->order.size(); i > 1; --i) std::swap(in->order[i - 1], in->order[rng() % i]);
  }
  return 0;
}

// density of every voxel and parent's first values
inline void density(const Input& in, std::vector<int32_t>* dens, std::vector<uint32_t>* parent) {
  dens->assign((size_t)in.M, 0);
  parent->assign((size_t)in.M, kClusterNone);
  for (uint32_t v : in.order) {
    (*dens)[v] = cluster_density(in.g, &in.keys[3 * (size_t)v], &in.cent[(size_t)kNormalsCent * v], in.q,
                                 in.weighted ? in.cnt.data() : nullptr);
    (*parent)[v] = cluster_seed(v, (*dens)[v], in.min_points);
  }
}

// `parent` as a plain array: one thread
struct PlainMem {
  uint32_t* p;
  uint32_t load(uint32_t i) const { return p[i]; }
  uint32_t cas(uint32_t i, uint32_t expected, uint32_t value) {
    const uint32_t was = p[i];
    if (was == expected) p[i] = value;
    return was;
  }
  void lower(uint32_t i, uint32_t value) {
    if (value < p[i]) p[i] = value;
  }
};

}  // namespace cluster_input
