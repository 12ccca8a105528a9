// Host build of the scalar core of the registration against the voxel cloud (csrc/register_core.hpp, which includes
// normals_core.hpp and voxel_core.hpp), for tests/test_registration_cpu.py.  Built with -ffp-contract=off.  The
// harness computes; the comparison with tests/registration.py is the test's.
//   register_host <in> <out>
//   in:  h, origin[3], max_distance, normals_radius, tol_rotation, tol_translation, init[16] (24 f64);
//        M, N, max_nn, max_iterations, log2 of the table size (5 i64); keys (M, 3) i32; centroids (M, 3) f64;
//        source (N, 3) f64
//   out: normals (M, 4) f64; counts (M,) i32; pairs, iterations, status, N (4 i64); transformation (16 f64); then
//        per iteration: the history row (8 f64), the 28 sums (f64), ids (N,) i32, d2 (N,) f64
// The steps are the device's: the table built with the filter's probe sequence, the normals of every voxel, then per
// iteration the nearest voxel of every moved point, the leaves summed by the adjacent-pair tree over the padded
// power of two, and register_step.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "device_standins.hpp"
#include "plane_core.hpp"
#include "register_core.hpp"
using namespace mc;

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> d;
  if (FILE* fp = std::fopen(path, "rb")) {
    uint8_t buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) d.insert(d.end(), buf, buf + k);
    std::fclose(fp);
  }
  return d;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::vector<uint8_t> in = slurp(argv[1]);
  if (in.size() < 232) return 2;
  double par[24];
  int64_t dim[5];
  std::memcpy(par, in.data(), 192);
  std::memcpy(dim, in.data() + 192, 40);
  const int64_t M = dim[0], N = dim[1];
  const int32_t max_nn = (int32_t)dim[2], max_iterations = (int32_t)dim[3];
  const int log2cap = (int)dim[4];
  if (M < 0 || N < 1 || max_iterations < 1 || log2cap < 6 || log2cap > 30 || ((int64_t)1 << log2cap) < 2 * M) return 2;
  if (max_nn != 0 && (max_nn < kNormalsMinNN || max_nn > kNormalsMaxNN)) return 2;
  if (in.size() != 232 + (size_t)M * 36 + (size_t)N * 24) return 2;
  const double h = par[0], *o = par + 1, max_distance = par[4], radius = par[5];
  if (!(max_distance / h <= kNormalsMaxR) || !(radius / h <= kNormalsMaxR)) return 2;
  std::vector<int32_t> keys((size_t)3 * M + 1);
  std::vector<double> c3((size_t)3 * M + 1), src((size_t)3 * N);
  if (M) {
    std::memcpy(keys.data(), in.data() + 232, (size_t)12 * M);
    std::memcpy(c3.data(), in.data() + 232 + (size_t)12 * M, (size_t)24 * M);
  }
  std::memcpy(src.data(), in.data() + 232 + (size_t)36 * M, (size_t)24 * N);

  // the build's table
  const size_t cap = (size_t)1 << log2cap;
  std::vector<unsigned long long> table(cap, kVoxelEmpty);
  std::vector<uint32_t> vid(cap, 0xDEADBEEFu);
  std::vector<double> cent((size_t)kNormalsCent * M + 1, 0.0);
  NormalsGrid g;
  g.shift = 64 - log2cap;
  g.mask = (uint32_t)(cap - 1);
  for (int64_t v = 0; v < M; ++v) {
    const uint64_t key = voxel_pack(&keys[3 * v]);
    uint32_t at = voxel_slot_first(key, g.shift, g.mask);
    while (table[at] != kVoxelEmpty) {
      if (table[at] == key) return 3;   // one voxel per cell
      at = voxel_slot_next(at, g.mask);
    }
    table[at] = key;
    vid[at] = (uint32_t)v;
    for (int a = 0; a < 3; ++a) cent[kNormalsCent * v + a] = c3[3 * v + a];
  }
  g.keys = table.data();
  g.vid = vid.data();
  g.cent = cent.data();

  // the normals of every voxel, as the window and cap kernels compute them
  NormalsQuery nq;
  nq.R = (int32_t)std::ceil(radius / h);
  if (nq.R < 1) nq.R = 1;
  nq.max_nn = max_nn;
  nq.r2 = radius * radius;
  std::vector<double> normals((size_t)4 * M + 1, 0.0), list_d2(kNormalsMaxNN);
  std::vector<uint16_t> list_ix(kNormalsMaxNN);
  std::vector<int32_t> counts((size_t)M + 1, 0);
  for (int64_t v = 0; v < M; ++v) {
    const int32_t* ki = &keys[3 * v];
    const double* ci = &cent[kNormalsCent * v];
    NormalsMoments m;
    int32_t n = normals_gather(g, ki, ci, nq, &m);
    if (nq.max_nn != 0 && n > nq.max_nn) {
      double last_d2;
      int32_t last_ix;
      normals_select(g, ki, ci, nq, list_d2.data(), list_ix.data(), 1, &last_d2, &last_ix);
      n = normals_gather_capped(g, ki, ci, nq, last_d2, last_ix, &m);
    }
    double C[6];
    normals_covariance(m, n, C);
    normals_finish(C, n, ci, false, 0.0, 0.0, 0.0, &normals[4 * v]);
    counts[v] = n;
  }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  if (M) {
    std::fwrite(normals.data(), 8, (size_t)4 * M, out);
    std::fwrite(counts.data(), 4, (size_t)M, out);
  }
  const long head = std::ftell(out);
  int64_t stats[4] = {0, 0, -1, N};
  double transformation[16] = {0};
  std::fwrite(stats, 8, 4, out);
  std::fwrite(transformation, 8, 16, out);

  RegPose T;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) T.R[3 * r + k] = par[8 + 4 * r + k];
    T.t[r] = par[8 + 4 * r + 3];
  }
  if (!register_pose_ok(T)) return 4;
  NormalsQuery w;
  w.R = (int32_t)std::ceil(max_distance / h);
  if (w.R < 1) w.R = 1;
  w.max_nn = 0;
  w.r2 = max_distance * max_distance;
  const int64_t L = plane_leaves(N);
  std::vector<double> leaves((size_t)kRegSums * L), d2((size_t)N);
  std::vector<int32_t> ids((size_t)N);
  int status = kRegGoOn;
  int32_t it = 0;
  int64_t pairs = 0;
  while (status == kRegGoOn && it < max_iterations) {
    std::fill(leaves.begin(), leaves.end(), 0.0);
    pairs = 0;
    for (int64_t i = 0; i < N; ++i) {
      double q[3];
      register_move(T, &src[3 * i], q);
      ids[i] = -1;
      d2[i] = (double)INFINITY;
      if (M > 0) register_nearest(g, h, o, w, q, &ids[i], &d2[i]);
      const bool pair = ids[i] >= 0 && counts[ids[i]] >= kNormalsMinNN;
      const double zero[3] = {0.0, 0.0, 0.0};
      double leaf[kRegSums];
      register_leaf(pair, pair ? q : zero, pair ? &cent[(size_t)kNormalsCent * ids[i]] : zero, pair ? &normals[(size_t)4 * ids[i]] : zero,
                    leaf);
      for (int c = 0; c < kRegSums; ++c) leaves[(size_t)c * L + i] = leaf[c];
      pairs += pair;
    }
    double sums[kRegSums], row[kRegHistory];
    for (int c = 0; c < kRegSums; ++c) sums[c] = plane_tree(leaves.data() + (size_t)c * L, L, 1);
    status = register_step(sums, pairs, par[6], par[7], &T, row);
    ++it;
    std::fwrite(row, 8, kRegHistory, out);
    std::fwrite(sums, 8, kRegSums, out);
    std::fwrite(ids.data(), 4, (size_t)N, out);
    std::fwrite(d2.data(), 8, (size_t)N, out);
  }
  if (status == kRegGoOn) status = kRegMaxIter;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) transformation[4 * r + k] = T.R[3 * r + k];
    transformation[4 * r + 3] = T.t[r];
  }
  transformation[15] = 1.0;
  stats[0] = pairs;
  stats[1] = it;
  stats[2] = status;
  std::fseek(out, head, SEEK_SET);
  std::fwrite(stats, 8, 4, out);
  std::fwrite(transformation, 8, 16, out);
  std::fclose(out);
  return 0;
}
