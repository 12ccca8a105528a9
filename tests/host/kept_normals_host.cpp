// Host build of the kept normals' marking (csrc/normals_core.hpp "kept normals": normals_next_epoch, normals_claim,
// normals_mark_window), for tests/test_kept_normals_cpu.py.  The harness marks; the comparison with
// tests/keptnormals.py is the test's.
//   kept_normals_host <in> <out>
//   in:  M, R, log2 of the table size, the epoch of the edit before the first (0: none yet), the number of edits
//        (5 i64); keys (M, 3) i32; then per edit: n (i64) and the voxel ids of its n items (u32), a voxel as often
//        as items land in it
//   out: per edit: the epoch it ran at, whether the stamps were cleared first, the touched voxels claimed, the dirty
//        voxels listed (4 i64), then the listed ids (u32) in the order they were claimed
// The table is built as tests/host/normals_host.cpp builds it; the stamps live across the edits as on the device,
// with a plain swap where the device has atomicExch.  An edit does what k_nrm_mark does per item: the first claim of
// the item's voxel walks the window of its cell and lists every voxel it is first to claim.
#include <algorithm>
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

struct Stamps {
  std::vector<uint32_t>& w;
  uint32_t exchange(uint32_t v, uint32_t epoch) {
    const uint32_t old = w.at(v);
    w[v] = epoch;
    return old;
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::vector<uint8_t> in = slurp(argv[1]);
  if (in.size() < 40) return 2;
  int64_t dim[5];
  std::memcpy(dim, in.data(), 40);
  const int64_t M = dim[0], edits = dim[4];
  const int32_t R = (int32_t)dim[1];
  const int log2cap = (int)dim[2];
  if (M < 0 || R < 1 || R > kNormalsMaxR || log2cap < 6 || log2cap > 30 || ((int64_t)1 << log2cap) < 2 * M) return 2;
  if (dim[3] < 0 || dim[3] > (int64_t)kNormalsEpochLast || edits < 0) return 2;
  size_t at_byte = 40 + (size_t)12 * M;
  if (in.size() < at_byte) return 2;
  std::vector<int32_t> keys((size_t)3 * M);
  if (M) std::memcpy(keys.data(), in.data() + 40, (size_t)12 * M);
  const size_t cap = (size_t)1 << log2cap;
  std::vector<unsigned long long> table(cap, kVoxelEmpty);
  std::vector<uint32_t> vid(cap, 0xDEADBEEFu);
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
  }
  g.keys = table.data();
  g.vid = vid.data();
  g.cent = nullptr;   // the marking reads no centroid
  std::vector<uint32_t> touched_w((size_t)M, 0u), dirty_w((size_t)M, 0u);
  Stamps touched = {touched_w}, dirty = {dirty_w};
  uint32_t epoch = (uint32_t)dim[3];
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (int64_t e = 0; e < edits; ++e) {
    int64_t n = 0;
    if (in.size() < at_byte + 8) return 2;
    std::memcpy(&n, in.data() + at_byte, 8);
    at_byte += 8;
    if (n < 0 || in.size() < at_byte + (size_t)4 * n) return 2;
    std::vector<uint32_t> items((size_t)n);
    if (n) std::memcpy(items.data(), in.data() + at_byte, (size_t)4 * n);
    at_byte += (size_t)4 * n;
    bool clear = false;
    epoch = normals_next_epoch(epoch, &clear);
    if (clear) {
      std::fill(touched_w.begin(), touched_w.end(), 0u);
      std::fill(dirty_w.begin(), dirty_w.end(), 0u);
    }
    std::vector<uint32_t> list;
    int64_t claimed = 0;
    for (uint32_t v : items) {
      if ((int64_t)v >= M) return 2;
      if (!normals_claim(touched, v, epoch)) continue;
      ++claimed;
      normals_mark_window(g, &keys[3 * (size_t)v], R, epoch, dirty, [&](uint32_t u) { list.push_back(u); });
    }
    const int64_t head[4] = {(int64_t)epoch, clear ? 1 : 0, claimed, (int64_t)list.size()};
    std::fwrite(head, sizeof head, 1, out);
    if (!list.empty()) std::fwrite(list.data(), sizeof(uint32_t), list.size(), out);
  }
  std::fclose(out);
  return at_byte == in.size() ? 0 : 2;
}
