// Host build of the scalar core of the voxel cloud's plane segmentation (csrc/plane_core.hpp), for
// tests/test_planes_cpu.py.  Built with -ffp-contract=off.  The harness computes; the comparison with
// tests/planes.py is the test's.
//   plane_host <in> <out>
//   in:  t (f64); K, seed, refine, M, has_among (5 x u64); cent (M, 3) f64; among (M,) u8 when has_among
//   out: scores (K,) i64; iteration, score, n_inliers, refined (4 x i64); samples (3,) i32 and a pad word;
//        model (4,) f64; cov (6,) f64; sums (9,) f64; hypothesis inliers (M,) u8; inliers (M,) u8
//   plane_host sampler <n> <count>   exit 0 when hypotheses 0 .. count - 1 of seeds 0 and 2^64 - 1 draw three distinct
//                                    places below n
// The steps are the device's: ids by a scan of the mask, the hypothesis table, the scores per hypothesis, the
// pick, the mask, the leaves summed by the adjacent-pair tree over the padded power of two, the refit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "device_standins.hpp"
#include "plane_core.hpp"
using namespace mc;

static int sampler(uint64_t n, uint32_t count) {
  const uint64_t seeds[2] = {0ull, ~0ull};
  for (uint64_t seed : seeds)
    for (uint32_t k = 0; k < count; ++k) {
      uint64_t at[3];
      plane_sample(seed, k, n, at);
      if (at[0] >= n || at[1] >= n || at[2] >= n) return 3;
      if (at[0] == at[1] || at[0] == at[2] || at[1] == at[2]) return 4;
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "sampler")
    return sampler(std::strtoull(argv[2], nullptr, 10), (uint32_t)std::strtoul(argv[3], nullptr, 10));
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  double t;
  uint64_t head[5];
  if (std::fread(&t, 8, 1, f) != 1 || std::fread(head, 8, 5, f) != 5) return 2;
  const int32_t K = (int32_t)head[0];
  const uint64_t seed = head[1];
  const bool refine = head[2] != 0;
  const int64_t M = (int64_t)head[3];
  const bool has_among = head[4] != 0;
  std::vector<double> cent((size_t)3 * M);
  std::vector<uint8_t> among((size_t)M, 1);
  if (std::fread(cent.data(), 8, cent.size(), f) != cent.size()) return 2;
  if (has_among && std::fread(among.data(), 1, among.size(), f) != among.size()) return 2;
  std::fclose(f);

  std::vector<uint32_t> ids;
  for (int64_t v = 0; v < M; ++v)
    if (among[v]) ids.push_back((uint32_t)v);
  const uint64_t n = ids.size();
  if (n < 3) return 5;
  const double tt = t * t;
  std::vector<PlaneHyp> hyp((size_t)K);
  std::vector<int32_t> smp((size_t)3 * K);
  for (int32_t k = 0; k < K; ++k) {
    uint64_t at[3];
    plane_sample(seed, (uint32_t)k, n, at);
    for (int j = 0; j < 3; ++j) smp[3 * (size_t)k + j] = (int32_t)ids[at[j]];
    hyp[k] = plane_hypothesis(&cent[3 * (size_t)smp[3 * (size_t)k]], &cent[3 * (size_t)smp[3 * (size_t)k + 1]],
                              &cent[3 * (size_t)smp[3 * (size_t)k + 2]], tt);
  }
  std::vector<uint32_t> score((size_t)K, 0);
  for (int32_t k = 0; k < K; ++k) {
    const PlaneHyp& h = hyp[k];
    for (uint32_t v : ids)
      if (plane_inlier(h.n[0], h.n[1], h.n[2], h.d, h.tau, cent[3 * (size_t)v], cent[3 * (size_t)v + 1], cent[3 * (size_t)v + 2]))
        ++score[k];
  }
  const int32_t k = plane_pick(score.data(), K);
  int64_t stats[4] = {-1, 0, 0, 0};
  int32_t samples[4] = {-1, -1, -1, 0};
  double model[4] = {0, 0, 0, 0}, cov[6] = {0, 0, 0, 0, 0, 0}, sums[kPlaneSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint8_t> first((size_t)M, 0), last((size_t)M, 0);
  if (k >= 0) {
    const PlaneHyp& h = hyp[k];
    int64_t n_in = 0;
    for (int64_t v = 0; v < M; ++v) {
      first[v] = among[v] && plane_inlier(h.n[0], h.n[1], h.n[2], h.d, h.tau, cent[3 * v], cent[3 * v + 1], cent[3 * v + 2]);
      n_in += first[v];
    }
    if (n_in != (int64_t)score[k]) return 6;
    stats[0] = k;
    stats[1] = score[k];
    for (int j = 0; j < 3; ++j) samples[j] = smp[3 * (size_t)k + j];
    last = first;
    if (refine) {
      const int64_t L = plane_leaves(M);
      std::vector<double> leaves((size_t)kPlaneSums * L, 0.0);
      for (int64_t v = 0; v < M; ++v) {
        double leaf[kPlaneSums];
        plane_leaf(first[v] != 0, &cent[3 * v], h.p0, leaf);
        for (int c = 0; c < kPlaneSums; ++c) leaves[(size_t)c * L + v] = leaf[c];
      }
      for (int c = 0; c < kPlaneSums; ++c) sums[c] = plane_tree(leaves.data() + (size_t)c * L, L, 1);
      plane_refit(sums, (int32_t)n_in, h.p0, model, cov);
      n_in = 0;
      for (int64_t v = 0; v < M; ++v) {
        last[v] = among[v] && plane_within(model[0], model[1], model[2], model[3], t, cent[3 * v], cent[3 * v + 1], cent[3 * v + 2]);
        n_in += last[v];
      }
      stats[3] = 1;
    } else {
      plane_model(h, model);
    }
    stats[2] = n_in;
  }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::vector<int64_t> wide(score.begin(), score.end());
  std::fwrite(wide.data(), 8, wide.size(), out);
  std::fwrite(stats, 8, 4, out);
  std::fwrite(samples, 4, 4, out);
  std::fwrite(model, 8, 4, out);
  std::fwrite(cov, 8, 6, out);
  std::fwrite(sums, 8, kPlaneSums, out);
  if (M) {
    std::fwrite(first.data(), 1, (size_t)M, out);
    std::fwrite(last.data(), 1, (size_t)M, out);
  }
  std::fclose(out);
  return 0;
}
