// The per-pair core of the ray-march scanner (csrc/raymarch_core.hpp) compiled for the CPU:
// tests/test_raymarch_cpu.py builds this file with -fsanitize=address,undefined -ffp-contract=off and
// runs it on the golden cases.
//
// Input file (little-endian): int64 F, n_rays, K, E; double step; steps[K]; dirs[n_rays][3];
// scene xyz[E][3]; int64 object[E]; then per frame origin[3], R[9].
// Output: one line "step object scene_index" per (frame, ray) (-1 -1 -1 for a miss), then
// "bad N": N = rays whose result differs between one scene chunk and chunks of 777 points merged by
// key order (the device's merge).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <math.h>
#include <stdint.h>
#include <vector>

#include "raymarch_core.hpp"

using namespace mcray;

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

static RayKey march(const Ray& r, const RayMarch& m, const std::vector<double>& steps, const std::vector<double>& xyz,
                    const std::vector<int64_t>& obj, int64_t e0, int64_t e1) {
  RayKey best{kRayMiss, kRayMiss, kRayMiss};
  double s_max = m.s_hi;
  for (int64_t e = e0; e < e1; ++e) {
    double s;
    if (ray_tube(r, m, xyz[3 * e], xyz[3 * e + 1], xyz[3 * e + 2], s) && ray_in_range(m, s_max, s)) {
      ray_exact(r, m, steps.data(), xyz[3 * e], xyz[3 * e + 1], xyz[3 * e + 2], s, (uint32_t)obj[e], (uint64_t)e, best);
      s_max = ray_s_max(m, steps.data(), best);
    }
  }
  return best;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  const std::vector<int64_t> hdr = read_n<int64_t>(f, 4);
  const int64_t F = hdr[0], n_rays = hdr[1], K = hdr[2], E = hdr[3];
  const double step = read_n<double>(f, 1)[0];
  const std::vector<double> steps = read_n<double>(f, K), dirs = read_n<double>(f, 3 * n_rays);
  const std::vector<double> xyz = read_n<double>(f, 3 * E);
  const std::vector<int64_t> obj = read_n<int64_t>(f, E);
  const RayMarch m = make_ray_march(steps.data(), (int32_t)K, step);
  long bad = 0;
  for (int64_t fr = 0; fr < F; ++fr) {
    const std::vector<double> pose = read_n<double>(f, 12);
    for (int64_t i = 0; i < n_rays; ++i) {
      Ray r;
      r.ox = pose[0]; r.oy = pose[1]; r.oz = pose[2];
      ray_rotate(pose.data() + 3, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], r.wx, r.wy, r.wz);
      RayKey whole{kRayMiss, kRayMiss, kRayMiss};
      if (K > 0) whole = march(r, m, steps, xyz, obj, 0, E);
      RayKey merged{kRayMiss, kRayMiss, kRayMiss};
      for (int64_t e0 = 0; K > 0 && e0 < E; e0 += 777) {
        const RayKey part = march(r, m, steps, xyz, obj, e0, e0 + 777 < E ? e0 + 777 : E);
        if (ray_key_less(part, merged)) merged = part;
      }
      if (merged.ko != whole.ko || merged.dist != whole.dist || merged.idx != whole.idx) ++bad;
      if (whole.ko == kRayMiss) printf("-1 -1 -1\n");
      else printf("%d %d %lld\n", (int)(whole.ko >> 32), (int)(uint32_t)whole.ko, (long long)whole.idx);
    }
  }
  fclose(f);
  printf("bad %ld\n", bad);
  return bad ? 1 : 0;
}
