// voxel_insert_host.cpp — the scalar rules of growing a voxel cloud (csrc/voxel_core.hpp: voxel_table_log2,
// voxel_record_ok) as the device compiles them, for tests/test_voxel_insert_cpu.py.  argv[1]: a file of cases, one
// per line; one answer per line on stdout:
//   g M n log2cap                  -> the log2 of the table's slots after the rule
//   r kx ky kz n Sx Sy Sz SI       -> 1: the record is accepted, 0: refused
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
    if (kind == 'g') {
      int64_t M, n;
      int log2cap;
      if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %d", &M, &n, &log2cap) != 3) { status = 2; break; }
      std::printf("%d\n", mc::voxel_table_log2(M, n, log2cap));
    } else if (kind == 'r') {
      int32_t k[3];
      int64_t n, S[3], SI;
      if (std::fscanf(f, "%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &k[0], &k[1],
                      &k[2], &n, &S[0], &S[1], &S[2], &SI) != 8) { status = 2; break; }
      std::printf("%d\n", mc::voxel_record_ok(k, n, S, SI) ? 1 : 0);
    } else {
      status = 2;
      break;
    }
  }
  std::fclose(f);
  return status;
}
