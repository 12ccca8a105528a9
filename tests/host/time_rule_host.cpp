// Host driver of csrc/time_rule.hpp for tests/test_time_rule_cpu.py.
//   in : int64 F, then per frame int64 n and n int32 stored times
//   out: per frame int32 even, t0, dt, then n int32: what the rule generates for index 0 .. n - 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "time_rule.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = std::fopen(argv[1], "rb");
  FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) return 3;
  int64_t F = 0;
  if (std::fread(&F, sizeof(F), 1, fi) != 1) return 4;
  for (int64_t f = 0; f < F; ++f) {
    int64_t n = 0;
    if (std::fread(&n, sizeof(n), 1, fi) != 1 || n < 0) return 5;
    std::vector<int32_t> t((size_t)n);
    if (n && std::fread(t.data(), sizeof(int32_t), (size_t)n, fi) != (size_t)n) return 6;
    int32_t head[3];
    head[0] = mc::time_rule_frame(t.data(), n, &head[1], &head[2]);
    std::vector<int32_t> gen((size_t)n);
    for (int64_t i = 0; i < n; ++i) gen[(size_t)i] = mc::time_rule_at(head[1], head[2], i);
    std::fwrite(head, sizeof(int32_t), 3, fo);
    if (n) std::fwrite(gen.data(), sizeof(int32_t), (size_t)n, fo);
  }
  std::fclose(fi);
  return std::fclose(fo) == 0 ? 0 : 7;
}
