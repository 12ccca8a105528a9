// voxel_remove_host.cpp — the scalar rules of shrinking a voxel cloud (csrc/voxel_core.hpp: voxel_table_shrink_log2,
// voxel_remainder_ok) as the device compiles them, for tests/test_voxel_remove_cpu.py.  argv[1]: a file of cases, one
// per line; one answer per line on stdout:
//   s M_keep log2cap               -> the log2 of the table's slots after the rule
//   m n Sx Sy Sz SI                -> 1: the record may be left behind, 0: no set of points sums to it
#include "voxel_core.hpp"

#include <cinttypes>
#include <cstdio>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char kind;
  int status = 0;
  while (std::fscanf(f, " %c", &kind) == 1) {
    if (kind == 's') {
      int64_t M;
      int log2cap;
      if (std::fscanf(f, "%" SCNd64 " %d", &M, &log2cap) != 2) { status = 2; break; }
      std::printf("%d\n", mc::voxel_table_shrink_log2(M, log2cap));
    } else if (kind == 'm') {
      int64_t n, S[3], SI;
      if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &n, &S[0], &S[1], &S[2], &SI) != 5) {
        status = 2;
        break;
      }
      std::printf("%d\n", mc::voxel_remainder_ok(n, S, SI) ? 1 : 0);
    } else {
      status = 2;
      break;
    }
  }
  std::fclose(f);
  return status;
}
