// Host harness of csrc/relfold.hpp (tests/test_relative_cpu.py): the fold of the relative SLERP
// deskew, compiled with g++ -ffp-contract=off from the header the device code includes.
//   relfold_host <in> <out>
// in:  int64 n, then q_ref[4], pos_ref[3], then n records of q0[4], v[4], p0[3], dp[3] (float64)
// out: the n folded records, same layout
#include <cstdint>
#include <cstdio>
#include <vector>

#include "relfold.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n = 0;
  double ref[7];
  if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > (1 << 24)) return 4;
  if (std::fread(ref, sizeof(double), 7, f) != 7) return 4;
  std::vector<double> rec((size_t)n * 14);
  if (std::fread(rec.data(), sizeof(double), rec.size(), f) != rec.size()) return 4;
  std::fclose(f);
  for (int64_t i = 0; i < n; ++i) {
    double* r = rec.data() + 14 * i;
    mc::rel_fold(ref, ref + 4, r, r + 4, r + 8, r + 11);
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(rec.data(), sizeof(double), rec.size(), f) != rec.size()) return 5;
  return std::fclose(f) == 0 ? 0 : 5;
}
