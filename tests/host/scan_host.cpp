// The decision core of the scene scanner (csrc/scan_core.hpp: ScanParams .. scan_visible) compiled for
// the CPU: tests/test_scan_edges_cpu.py builds this file with -fsanitize=address,undefined
// -ffp-contract=off and runs it on the edge scenes of tests/scanedges.py.
//
// Input file (little-endian doubles): the number of cases, then per case range_min, range_max,
// fov_horizontal, fov_vertical (the config's values; prepared below as mc_scan_count prepares them);
// the pose R[9] row-major, t[3]; the point count E; xyz[E][3].
// Output: one line "visible exact" per point, the cases back to back: scan_visible's result and
// how many of atan2 / asin it evaluated (0: the fast tier or a range test decided).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <math.h>
#include <stdint.h>
#include <vector>

// the exact tier's calls, counted: defined after <math.h> and before the core, whose text they rename
static int g_exact = 0;
static double counted_atan2(double y, double x) { ++g_exact; return atan2(y, x); }
static double counted_asin(double x) { ++g_exact; return asin(x); }
#define atan2 counted_atan2
#define asin counted_asin

#include "scan_core.hpp"
using namespace mc;

static std::vector<double> read_n(FILE* f, size_t n) {
  std::vector<double> v(n);
  if (n && fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  double n_cases = 0;
  if (fread(&n_cases, sizeof(double), 1, f) != 1) { fprintf(stderr, "short input\n"); return 2; }
  for (int64_t c = 0; c < (int64_t)n_cases; ++c) {
    const std::vector<double> cfg = read_n(f, 4), pose = read_n(f, 12);
    const int64_t E = (int64_t)read_n(f, 1)[0];
    const std::vector<double> xyz = read_n(f, 3 * (size_t)E);
    // mc_scan_count's preparation: LMC:715 max_range_sq, LMC:740-741 half FOVs
    const double par[4] = {cfg[0], cfg[1] * cfg[1], cfg[2] / 2, cfg[3] / 2};
    const ScanParams sp = make_scan_params(par, 1);
    for (int64_t e = 0; e < E; ++e) {
      double lx, ly, lz;
      g_exact = 0;
      const bool v = scan_visible(pose.data(), xyz[3 * e], xyz[3 * e + 1], xyz[3 * e + 2], sp, lx, ly, lz);
      printf("%d %d\n", v ? 1 : 0, g_exact);
    }
  }
  fclose(f);
  return 0;
}
