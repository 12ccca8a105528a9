// Host build of the per-record cores of the LAS codec (csrc/las_core.hpp), for tests/test_las_host.py.
// Built with -ffp-contract=off so that the only fused multiply-add is one the source asks
// for.  The harness computes; the comparison with tests/las.py is the test's, bit for bit.
//   las_host enc <in> <out>   in: scale[3], off[3], imul, tmul (8 f64), then rows of 5 f64
//                             out: per row X[3] (i32), intensity (u32), gps (f64), bad (i32), 0 (i32)
//   las_host dec <in> <out>   in: format, record length (2 i64), scale[3], off[3] (6 f64), then the records
//                             out: per record x, y, z, intensity, gps (5 f64), time ns (i64), fits (i64)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "las_core.hpp"
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
  if (!out) return 2;
  if (!std::strcmp(argv[1], "enc")) {
    if (in.size() < 64 || (in.size() - 64) % 40) return 2;
    double par[8];
    std::memcpy(par, in.data(), 64);
    const size_t n = (in.size() - 64) / 40;
    for (size_t i = 0; i < n; ++i) {
      double c[5];
      std::memcpy(c, in.data() + 64 + 40 * i, 40);
      const LasRec r = las_encode_rec(c, par, par + 3, par[6], par[7]);
      struct { int32_t X[3]; uint32_t it; double gps; int32_t bad, zero; } o = {{r.X[0], r.X[1], r.X[2]}, r.intensity, r.gps, r.bad, 0};
      static_assert(sizeof o == 32, "packed");
      std::fwrite(&o, sizeof o, 1, out);
    }
  } else if (!std::strcmp(argv[1], "dec")) {
    if (in.size() < 64) return 2;
    int64_t fr[2];
    double par[6];
    std::memcpy(fr, in.data(), 16);
    std::memcpy(par, in.data() + 16, 48);
    if (fr[1] < 20 || (in.size() - 64) % (size_t)fr[1]) return 2;
    const size_t n = (in.size() - 64) / (size_t)fr[1];
    for (size_t i = 0; i < n; ++i) {
      double v[5];
      las_decode_rec(in.data() + 64 + (size_t)fr[1] * i, (int)fr[0], par, par + 3, v);
      int64_t t[2] = {0, 0};
      t[1] = las_time_ns(v[4], &t[0]) ? 1 : 0;
      std::fwrite(v, 8, 5, out);
      std::fwrite(t, 8, 2, out);
    }
  } else {
    return 2;
  }
  std::fclose(out);
  return 0;
}
