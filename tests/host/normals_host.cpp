// Host build of the scalar core of the voxel cloud's surface normals (csrc/normals_core.hpp, which includes
// voxel_core.hpp), for tests/test_normals_cpu.py.  Built with -ffp-contract=off.
// The harness computes; the comparison with tests/normals.py is the test's.
//   normals_host <in> <out>
//   in:  h, radius, r2, viewpoint[3] (6 f64); M, R, max_nn, has_viewpoint, log2 of the table size (5 i64);
//        keys (M, 3) i32; centroids (M, 3) f64
//   out: per voxel n (i32), 0 (i32), C[6], nx ny nz curvature (f64), and the kept
//        cells of its window in walk order as 768 bits (12 u64)
// The table is built here with the filter's own probe sequence (voxel_slot_first / voxel_slot_next), the keys
// inserted in voxel order, so the chains of a small table are walked as on the device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "normals_core.hpp"
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
  if (in.size() < 88) return 2;
  double par[6];
  int64_t dim[5];
  std::memcpy(par, in.data(), 48);
  std::memcpy(dim, in.data() + 48, 40);
  const int64_t M = dim[0];
  const int log2cap = (int)dim[4];
  if (M < 0 || dim[1] < 1 || dim[1] > kNormalsMaxR || log2cap < 6 || log2cap > 30 || ((int64_t)1 << log2cap) < 2 * M) return 2;
  if (dim[2] != 0 && (dim[2] < kNormalsMinNN || dim[2] > kNormalsMaxNN)) return 2;
  if (in.size() != 88 + (size_t)M * (12 + 24)) return 2;
  std::vector<int32_t> keys((size_t)3 * M);
  std::vector<double> c3((size_t)3 * M);
  if (M) {
    std::memcpy(keys.data(), in.data() + 88, (size_t)12 * M);
    std::memcpy(c3.data(), in.data() + 88 + (size_t)12 * M, (size_t)24 * M);
  }
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
  NormalsQuery q;
  q.R = (int32_t)dim[1];
  q.max_nn = (int32_t)dim[2];
  q.r2 = par[2];
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::vector<double> list_d2(kNormalsMaxNN);
  std::vector<uint16_t> list_ix(kNormalsMaxNN);
  for (int64_t v = 0; v < M; ++v) {
    const int32_t* ki = &keys[3 * v];
    const double* ci = &cent[kNormalsCent * v];
    struct { int32_t n, zero; double C[6], o[4]; uint64_t kept[12]; } r;
    static_assert(sizeof r == 184, "packed");
    std::memset(&r, 0, sizeof r);
    NormalsMoments m;
    const int32_t found = normals_gather(g, ki, ci, q, &m);
    if (q.max_nn != 0 && found > q.max_nn) {
      double last_d2;
      int32_t last_ix;
      normals_select(g, ki, ci, q, list_d2.data(), list_ix.data(), 1, &last_d2, &last_ix);
      r.n = normals_gather_capped(g, ki, ci, q, last_d2, last_ix, &m);
      normals_neighbours(g, ki, ci, q, [&](int32_t ix, const double*, double d2) {
        if (!normals_before(last_d2, last_ix, d2, ix)) r.kept[ix >> 6] |= (uint64_t)1 << (ix & 63);
      });
    } else {
      r.n = found;
      normals_neighbours(g, ki, ci, q, [&](int32_t ix, const double*, double) { r.kept[ix >> 6] |= (uint64_t)1 << (ix & 63); });
    }
    normals_covariance(m, r.n, r.C);
    normals_finish(r.C, r.n, ci, dim[3] != 0, par[3], par[4], par[5], r.o);
    std::fwrite(&r, sizeof r, 1, out);
  }
  std::fclose(out);
  return 0;
}
