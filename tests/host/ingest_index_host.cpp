// Stand-alone driver of the host LVX walker (livox-motion-compensation-sim_amd/csrc/ingest_index.cpp),
// built with -fsanitize=address,undefined by tests/test_ingest_index_cpu.py: the walker reads
// untrusted bytes, so every output array is a heap block of exactly the size the interface asks for and
// the file itself sits in a heap block of exactly its length.  For each file named on the command
// line: probe, then (when the probe accepts it) index and check_layout, one report line
//   <path> ok <format> <frames>      or      <path> invalid <message>
// and then the same walk over every truncation of the file and over single-byte mutations of it, which
// must never disagree with itself (probe accepts, index refuses) or touch memory outside the blocks.
// Exit status 0 unless the walker contradicts itself.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "ingest_index.hpp"

static int walk(const uint8_t* src, int64_t n, char* msg, size_t msg_len, int* fmt_out, int32_t* F_out) {
  std::unique_ptr<uint8_t[]> file(new uint8_t[n > 0 ? n : 1]);   // exact size: a read past the end is a report
  if (n > 0) std::memcpy(file.get(), src, (size_t)n);
  int fmt = -1;
  int32_t F = -1;
  if (mcingest::probe(n > 0 ? file.get() : nullptr, n, &fmt, &F, msg, msg_len)) return 1;
  std::unique_ptr<int64_t[]> pos(new int64_t[F + 1]), slots(new int64_t[F > 0 ? F : 1]), ts(new int64_t[F > 0 ? F : 1]);
  std::unique_ptr<uint64_t[]> ids(new uint64_t[F > 0 ? F : 1]);
  mcingest::DeviceBlock dv;
  if (mcingest::index(file.get(), n, fmt, F, pos.get(), slots.get(), ids.get(), ts.get(), &dv, msg, msg_len)) return 2;
  if (mcingest::check_layout(fmt, n, F, pos.get(), slots.get(), msg, msg_len)) return 2;
  // what a decode launch would read: every slot's 14 bytes lie inside the file
  for (int32_t f = 0; f < F; ++f) {
    const int64_t body = pos[f + 1] - pos[f] - mcingest::frame_header_bytes(fmt);
    const int64_t need = fmt == mcingest::kFmtV11 ? slots[f] / 96 * 1366 : slots[f] * 14;
    if (body != need || pos[f + 1] > n) { std::snprintf(msg, msg_len, "frame %d: layout and slots disagree", f); return 2; }
  }
  *fmt_out = fmt;
  *F_out = F;
  return 0;
}

int main(int argc, char** argv) {
  int contradictions = 0;
  char msg[256];
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> data;
    if (FILE* fp = std::fopen(argv[a], "rb")) {
      uint8_t buf[65536];
      size_t k;
      while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) data.insert(data.end(), buf, buf + k);
      std::fclose(fp);
    } else {
      std::printf("%s unreadable\n", argv[a]);
      return 2;
    }
    int fmt = -1;
    int32_t F = -1;
    msg[0] = 0;
    const int r = walk(data.data(), (int64_t)data.size(), msg, sizeof msg, &fmt, &F);
    if (r == 0) std::printf("%s ok %d %d\n", argv[a], fmt, F);
    else std::printf("%s invalid %s\n", argv[a], msg);
    if (r == 2) ++contradictions;
    const int64_t n = (int64_t)data.size();
    for (int64_t cut = 0; cut < n; cut += cut < 3000 ? 1 : 97)
      if (walk(data.data(), cut, msg, sizeof msg, &fmt, &F) == 2) ++contradictions;
    std::mt19937_64 rng(n);
    std::vector<uint8_t> m(data);
    for (int it = 0; it < 3000 && n > 0; ++it) {
      const size_t at = it % 3 ? (size_t)(rng() % (uint64_t)(n < 400 ? n : 400)) : (size_t)(rng() % (uint64_t)n);
      const uint8_t keep = m[at];
      m[at] = (uint8_t)rng();
      if (walk(m.data(), n, msg, sizeof msg, &fmt, &F) == 2) ++contradictions;
      m[at] = keep;
    }
  }
  std::printf("contradictions %d\n", contradictions);
  return contradictions ? 1 : 0;
}
