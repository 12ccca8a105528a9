// The union-find of csrc/cluster_core.hpp under ThreadSanitizer, for tests/test_clusters_cpu.py: the same
// cluster_find / cluster_unite text the device compiles, with a std::atomic policy (relaxed, as the device's
// agent-scope atomics) on eight threads, thread t taking every eighth voxel of the input's order, against the
// plain-array policy on one thread.  Built with -fsanitize=thread -pthread -ffp-contract=off.
//   cluster_tsan_host <in>           (the input: cluster_input.hpp)
// Exit status 0 when every core voxel has the same root either way and parent[x] <= x holds; a race is
// ThreadSanitizer's report on stderr.
#include <atomic>
#include <thread>

#include "cluster_input.hpp"
using namespace mc;
using namespace cluster_input;

struct AtomicMem {
  std::atomic<uint32_t>* p;
  uint32_t load(uint32_t i) const { return p[i].load(std::memory_order_relaxed); }
  uint32_t cas(uint32_t i, uint32_t expected, uint32_t value) {
    p[i].compare_exchange_strong(expected, value, std::memory_order_relaxed);
    return expected;   // the word before, as atomicCAS returns it
  }
  void lower(uint32_t i, uint32_t value) {   // an atomic minimum
    uint32_t cur = p[i].load(std::memory_order_relaxed);
    while (value < cur && !p[i].compare_exchange_weak(cur, value, std::memory_order_relaxed)) {
    }
  }
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Input in;
  if (int r = read(argv[1], &in)) return r;
  const int64_t M = in.M;
  std::vector<int32_t> dens;
  std::vector<uint32_t> seed;
  density(in, &dens, &seed);
  auto unite_from = [&](auto& m, size_t first, size_t step) {
    for (size_t at = first; at < in.order.size(); at += step) {
      const uint32_t v = in.order[at];
      if (m.load(v) != kClusterNone)
        cluster_union_voxel(in.g, &in.keys[3 * (size_t)v], &in.cent[(size_t)kNormalsCent * v], in.q, m, v);
    }
  };
  std::vector<uint32_t> plain = seed;
  PlainMem one = {plain.data()};
  unite_from(one, 0, 1);
  std::vector<std::atomic<uint32_t>> shared((size_t)M);
  for (int64_t v = 0; v < M; ++v) shared[v].store(seed[v], std::memory_order_relaxed);
  constexpr int kThreads = 8;
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&, t] {
      AtomicMem m = {shared.data()};
      unite_from(m, (size_t)t, kThreads);
    });
  for (auto& t : threads) t.join();
  AtomicMem many = {shared.data()};
  int64_t differ = 0, above = 0, cores = 0;
  for (int64_t v = 0; v < M; ++v) {
    if (seed[v] == kClusterNone) {
      differ += many.load((uint32_t)v) != kClusterNone;
      continue;
    }
    ++cores;
    above += many.load((uint32_t)v) > (uint32_t)v;
    differ += cluster_find(many, (uint32_t)v) != cluster_find(one, (uint32_t)v);
  }
  std::printf("cores %lld differ %lld above %lld\n", (long long)cores, (long long)differ, (long long)above);
  return differ || above ? 1 : 0;
}
