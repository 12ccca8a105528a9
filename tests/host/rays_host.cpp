// Host build of the scalar core of the rays through the voxel cloud (csrc/rays_core.hpp, which includes
// normals_core.hpp and voxel_core.hpp), for tests/test_rays_cpu.py.  Built with -ffp-contract=off.  The harness
// computes; the comparison with tests/rays.py is the test's.
//   rays_host <in> <out>
//   in:  h, origin[3] (4 f64); M, N, n_origins (1 or N), guard, max_steps, log2 of the table size (6 i64);
//        keys (M, 3) i32; source (N, 3) f64; origins (n_origins, 3) f64
//   out: rays, skipped, steps, 0 (4 i64); passed (M,) i32; ended (M,) i32; through (N,) i32
// The steps are the device's: the table built with the filter's probe sequence, then rays_walk of every ray with
// callbacks that add 1 to the voxel's count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_standins.hpp"
#include "rays_core.hpp"
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
  if (in.size() < 80) return 2;
  double par[4];
  int64_t dim[6];
  std::memcpy(par, in.data(), 32);
  std::memcpy(dim, in.data() + 32, 48);
  const int64_t M = dim[0], N = dim[1], n_origins = dim[2];
  const int32_t guard = (int32_t)dim[3], max_steps = (int32_t)dim[4];
  const int log2cap = (int)dim[5];
  if (M < 0 || N < 1 || (n_origins != 1 && n_origins != N) || log2cap < 6 || log2cap > 30 || ((int64_t)1 << log2cap) < 2 * M) return 2;
  if (guard < 0 || guard > kRaysMaxGuard || max_steps < 1 || max_steps > kRaysMaxSteps) return 2;
  if (in.size() != 80 + (size_t)M * 12 + (size_t)N * 24 + (size_t)n_origins * 24) return 2;
  std::vector<int32_t> keys((size_t)3 * M + 1);
  std::vector<double> src((size_t)3 * N), origins((size_t)3 * n_origins);
  if (M) std::memcpy(keys.data(), in.data() + 80, (size_t)12 * M);
  std::memcpy(src.data(), in.data() + 80 + (size_t)12 * M, (size_t)24 * N);
  std::memcpy(origins.data(), in.data() + 80 + (size_t)12 * M + (size_t)24 * N, (size_t)24 * n_origins);

  // the build's table
  const size_t cap = (size_t)1 << log2cap;
  std::vector<unsigned long long> table(cap, kVoxelEmpty);
  std::vector<uint32_t> vid(cap, 0xDEADBEEFu);
  RaysGrid G = {};
  G.g.shift = 64 - log2cap;
  G.g.mask = (uint32_t)(cap - 1);
  for (int64_t v = 0; v < M; ++v) {
    const uint64_t key = voxel_pack(&keys[3 * v]);
    uint32_t at = voxel_slot_first(key, G.g.shift, G.g.mask);
    while (table[at] != kVoxelEmpty) {
      if (table[at] == key) return 3;   // one voxel per cell
      at = voxel_slot_next(at, G.g.mask);
    }
    table[at] = key;
    vid[at] = (uint32_t)v;
  }
  G.g.keys = table.data();
  G.g.vid = vid.data();
  G.g.cent = nullptr;   // never read
  G.M = M;
  G.h = par[0];
  for (int a = 0; a < 3; ++a) G.o[a] = par[1 + a];

  std::vector<int32_t> passed((size_t)M + 1, 0), ended((size_t)M + 1, 0), through((size_t)N);
  int64_t stats[4] = {N, 0, 0, 0};
  for (int64_t i = 0; i < N; ++i) {
    int32_t steps = 0;
    through[i] = rays_walk(
        G, &origins[3 * (n_origins == 1 ? 0 : i)], &src[3 * i], guard, max_steps,
        [&](uint32_t v) {
          if ((int64_t)v >= M) std::abort();
          passed[v] += 1;
        },
        [&](uint32_t v) {
          if ((int64_t)v >= M) std::abort();
          ended[v] += 1;
        },
        &steps);
    stats[1] += through[i] == kRaysSkipped;
    stats[2] += steps;
  }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(stats, 8, 4, out);
  if (M) {
    std::fwrite(passed.data(), 4, (size_t)M, out);
    std::fwrite(ended.data(), 4, (size_t)M, out);
  }
  std::fwrite(through.data(), 4, (size_t)N, out);
  std::fclose(out);
  return 0;
}
