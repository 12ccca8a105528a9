// Host build of the scalar core of the voxel cloud's density clustering (csrc/cluster_core.hpp, on top of
// normals_core.hpp's walker), for tests/test_clusters_cpu.py.  Built with -ffp-contract=off.
// The harness computes; the comparison with tests/clusters.py is the test's.
//   cluster_host <in> <out>          (the input: cluster_input.hpp)
//   out: labels (M,) i32; density (M,) i32; K (i64); voxels (K,) i32; points (K,) i64; cell_min (K, 3) i32;
//        cell_max (K, 3) i32
// Every phase visits the voxels in the input's order (forwards, backwards or shuffled) with the plain-array
// policy: the unions arrive in another order each time and the output may not change by a byte.
#include <climits>

#include "cluster_input.hpp"
using namespace mc;
using namespace cluster_input;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  Input in;
  if (int r = read(argv[1], &in)) return r;
  const int64_t M = in.M;
  std::vector<int32_t> dens;
  std::vector<uint32_t> parent;
  density(in, &dens, &parent);
  PlainMem m = {parent.data()};
  for (uint32_t v : in.order)
    if (m.load(v) != kClusterNone)
      cluster_union_voxel(in.g, &in.keys[3 * (size_t)v], &in.cent[(size_t)kNormalsCent * v], in.q, m, v);
  // the invariant: parent[x] <= x for every core voxel
  for (int64_t v = 0; v < M; ++v)
    if (parent[v] != kClusterNone && parent[v] > (uint32_t)v) return 4;
  std::vector<uint32_t> root((size_t)M);
  for (uint32_t v : in.order)
    root[v] = cluster_root_voxel(in.g, &in.keys[3 * (size_t)v], &in.cent[(size_t)kNormalsCent * v], in.q, m, v);
  // number: the roots in ascending voxel id
  std::vector<int32_t> number((size_t)M, kClusterNoise), labels((size_t)M, kClusterNoise);
  int64_t K = 0;
  for (int64_t v = 0; v < M; ++v)
    if (root[v] == (uint32_t)v) number[v] = (int32_t)K++;
  for (int64_t v = 0; v < M; ++v)
    if (root[v] != kClusterNone) {
      if (root[v] >= (uint32_t)M || number[root[v]] < 0) return 5;   // a root that is none
      labels[v] = number[root[v]];
    }
  std::vector<int32_t> voxels((size_t)K, 0), lo((size_t)3 * K, INT_MAX), hi((size_t)3 * K, INT_MIN);
  std::vector<int64_t> points((size_t)K, 0);
  for (uint32_t v : in.order) {
    const int32_t c = labels[v];
    if (c < 0) continue;
    ++voxels[c];
    points[c] += in.cnt[v];
    for (int a = 0; a < 3; ++a) {
      lo[3 * (size_t)c + a] = std::min(lo[3 * (size_t)c + a], in.keys[3 * (size_t)v + a]);
      hi[3 * (size_t)c + a] = std::max(hi[3 * (size_t)c + a], in.keys[3 * (size_t)v + a]);
    }
  }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  auto put = [&](const void* p, size_t size, size_t n) {   // an empty vector's data() may be null
    if (n) std::fwrite(p, size, n, out);
  };
  put(labels.data(), 4, (size_t)M);
  put(dens.data(), 4, (size_t)M);
  put(&K, 8, 1);
  put(voxels.data(), 4, (size_t)K);
  put(points.data(), 8, (size_t)K);
  put(lo.data(), 4, (size_t)3 * K);
  put(hi.data(), 4, (size_t)3 * K);
  std::fclose(out);
  return 0;
}
