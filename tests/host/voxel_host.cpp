// Host build of the scalar core of the voxel-grid filter (csrc/voxel_core.hpp), for tests/test_voxel_cpu.py.
// Built with -ffp-contract=off.
// The harness computes; the comparison with tests/voxel.py is the test's, bit for bit.
//   voxel_host quant <in> <out>   in: h, origin[3] (4 f64), then rows x, y, z, intensity (4 f64)
//                                 out: per row k[3] (i32), bad (i32), Q[3], QI (i64), key (u64),
//                                      the key unpacked again [3] (i32), 0 (i32)
//   voxel_host probe <in> <out>   in: 4 f64 (unused), log2 of the table size, the number of keys (2 u64), the keys
//                                 (u64), then slot indices (u64); out: voxel_slot_first of each key, then
//                                 voxel_slot_next of each slot index (u32)
//   voxel_host fin <in> <out>     in: h, origin[3] (4 f64), then per voxel k[3] (i32), 0 (i32), S[3], SI, n (i64)
//                                 out: per voxel cx, cy, cz, i (4 f64), then the same as 4 f32
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "voxel_core.hpp"
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
  if (argc != 4) return 2;
  const std::vector<uint8_t> in = slurp(argv[2]);
  FILE* out = std::fopen(argv[3], "wb");
  if (!out || in.size() < 32) return 2;
  double par[4];
  std::memcpy(par, in.data(), 32);
  if (!std::strcmp(argv[1], "quant")) {
    if ((in.size() - 32) % 32) return 2;
    const size_t n = (in.size() - 32) / 32;
    for (size_t i = 0; i < n; ++i) {
      double c[4];
      std::memcpy(c, in.data() + 32 + 32 * i, 32);
      const VoxelPoint r = voxel_quantise(c, c[3], par[0], par + 1);
      struct { int32_t k[3], bad; int64_t Q[3], QI; uint64_t key; int32_t uk[3], zero; } o;
      static_assert(sizeof o == 72, "packed");
      std::memset(&o, 0, sizeof o);
      for (int a = 0; a < 3; ++a) { o.k[a] = r.k[a]; o.Q[a] = r.Q[a]; }
      o.bad = r.bad;
      o.QI = r.QI;
      o.key = voxel_pack(r.k);
      voxel_unpack(o.key, o.uk);
      std::fwrite(&o, sizeof o, 1, out);
    }
  } else if (!std::strcmp(argv[1], "fin")) {
    if ((in.size() - 32) % 56) return 2;
    const size_t n = (in.size() - 32) / 56;
    for (size_t i = 0; i < n; ++i) {
      struct { int32_t k[3], zero; int64_t S[3], SI, n; } v;
      static_assert(sizeof v == 56, "packed");
      std::memcpy(&v, in.data() + 32 + 56 * i, 56);
      double c[4];
      voxel_finalise(v.k, v.S, v.SI, v.n, par[0], par + 1, c);
      const float f[4] = {(float)c[0], (float)c[1], (float)c[2], (float)c[3]};
      std::fwrite(c, 8, 4, out);
      std::fwrite(f, 4, 4, out);
    }
  } else if (!std::strcmp(argv[1], "probe")) {
    if (in.size() < 48) return 2;
    uint64_t head[2];
    std::memcpy(head, in.data() + 32, 16);
    const size_t nk = (size_t)head[1];
    if (head[0] < 1 || head[0] > 32 || (in.size() - 48) % 8 || (in.size() - 48) / 8 < nk) return 2;
    const size_t ns = (in.size() - 48) / 8 - nk;
    const int shift = 64 - (int)head[0];
    const uint32_t mask = (uint32_t)(((uint64_t)1 << head[0]) - 1);
    for (size_t i = 0; i < nk + ns; ++i) {
      uint64_t v;
      std::memcpy(&v, in.data() + 48 + 8 * i, 8);
      const uint32_t r = i < nk ? voxel_slot_first(v, shift, mask) : voxel_slot_next((uint32_t)v, mask);
      std::fwrite(&r, 4, 1, out);
    }
  } else {
    return 2;
  }
  std::fclose(out);
  return 0;
}
