// Host build of the frames of a batch registered together (csrc/register_core.hpp: the block map, the per-frame padded
// tree, the tail tree, the step and the freeze of an ended frame), for tests/test_register_frames_cpu.py.  Built with
// -ffp-contract=off.  The harness computes; the comparison with tests/registration.py, frame by frame, is the test's.
//   register_frames_host <in> <out>
//   in:  h, origin[3], max_distance, normals_radius, tol_rotation, tol_translation (8 f64);
//        M, N, F, max_nn, max_iterations, log2 of the table size (6 i64); counts (F,) i64; inits (F, 16) f64;
//        keys (M, 3) i32; centroids (M, 3) f64; source (N, 3) f64, frame-major
//   out: normals (M, 4) f64; counts (M,) i32; B (1 i64) and the frame of each of the B first-level blocks (i32);
//        per frame pairs, iterations, status, N_f (4 i64) and the transformation (16 f64); the history
//        (F, max_iterations, 8) f64; the iterations the loop ran (1 i64)
// The steps are the device's, launch by launch: k_rg_frames_step as a loop over the block map's workgroups (a
// workgroup of an ended frame or past the frame's last point does nothing; the tree scratch was zeroed once), a loop
// per further level, and the solve of every live frame; the loop ends when no frame is live.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "device_standins.hpp"
#include "register_core.hpp"
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

// plane_block_tree: a workgroup's 256 leaves of every sum -> out[c * stride]
static void block_tree(double x[kRegSums][kRegBlock], double* out, int64_t stride) {
  for (int c = 0; c < kRegSums; ++c) out[c * stride] = plane_tree(x[c], kRegBlock, 1);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::vector<uint8_t> in = slurp(argv[1]);
  if (in.size() < 112) return 2;
  double par[8];
  int64_t dim[6];
  std::memcpy(par, in.data(), 64);
  std::memcpy(dim, in.data() + 64, 48);
  const int64_t M = dim[0], N = dim[1], F = dim[2];
  const int32_t max_nn = (int32_t)dim[3], max_iterations = (int32_t)dim[4];
  const int log2cap = (int)dim[5];
  if (M < 0 || N < 0 || F < 0 || F > (1 << 20) || max_iterations < 1 || log2cap < 6 || log2cap > 30 || ((int64_t)1 << log2cap) < 2 * M)
    return 2;
  if (max_nn != 0 && (max_nn < kNormalsMinNN || max_nn > kNormalsMaxNN)) return 2;
  if (in.size() != 112 + (size_t)F * 136 + (size_t)M * 36 + (size_t)N * 24) return 2;
  const double h = par[0], *o = par + 1, max_distance = par[4], radius = par[5];
  if (!(max_distance / h <= kNormalsMaxR) || !(radius / h <= kNormalsMaxR)) return 2;
  std::vector<int64_t> counts_f((size_t)F + 1, 0);
  std::vector<double> inits((size_t)16 * F + 1);
  std::vector<int32_t> keys((size_t)3 * M + 1);
  std::vector<double> c3((size_t)3 * M + 1), src((size_t)3 * N + 1);
  const uint8_t* at = in.data() + 112;
  if (F) {
    std::memcpy(counts_f.data(), at, (size_t)8 * F);
    std::memcpy(inits.data(), at + (size_t)8 * F, (size_t)128 * F);
  }
  at += (size_t)136 * F;
  if (M) {
    std::memcpy(keys.data(), at, (size_t)12 * M);
    std::memcpy(c3.data(), at + (size_t)12 * M, (size_t)24 * M);
  }
  at += (size_t)36 * M;
  if (N) std::memcpy(src.data(), at, (size_t)24 * N);
  std::vector<int64_t> doff((size_t)F + 1, 0);
  for (int64_t f = 0; f < F; ++f) {
    if (counts_f[f] < 0) return 2;
    doff[f + 1] = doff[f] + counts_f[f];
  }
  if (doff[F] != N) return 2;

  // the build's table
  const size_t cap = (size_t)1 << log2cap;
  std::vector<unsigned long long> table(cap, kVoxelEmpty);
  std::vector<uint32_t> vid(cap, 0xDEADBEEFu);
  std::vector<double> cent((size_t)kNormalsCent * M + 1, 0.0);
  NormalsGrid g;
  g.shift = 64 - log2cap;
  g.mask = (uint32_t)(cap - 1);
  for (int64_t v = 0; v < M; ++v) {
    const uint64_t key = voxel_pack(&keys[3 * v]);
    uint32_t slot = voxel_slot_first(key, g.shift, g.mask);
    while (table[slot] != kVoxelEmpty) {
      if (table[slot] == key) return 3;   // one voxel per cell
      slot = voxel_slot_next(slot, g.mask);
    }
    table[slot] = key;
    vid[slot] = (uint32_t)v;
    for (int a = 0; a < 3; ++a) cent[kNormalsCent * v + a] = c3[3 * v + a];
  }
  g.keys = table.data();
  g.vid = vid.data();
  g.cent = cent.data();

  // the normals of every voxel, once
  NormalsQuery nq;
  nq.R = (int32_t)std::ceil(radius / h);
  if (nq.R < 1) nq.R = 1;
  nq.max_nn = max_nn;
  nq.r2 = radius * radius;
  std::vector<double> normals((size_t)4 * M + 1, 0.0), list_d2(kNormalsMaxNN);
  std::vector<uint16_t> list_ix(kNormalsMaxNN);
  std::vector<int32_t> counts((size_t)M + 1, 0);
  for (int64_t v = 0; v < M; ++v) {
    const int32_t* ki = &keys[3 * v];
    const double* ci = &cent[kNormalsCent * v];
    NormalsMoments m;
    int32_t n = normals_gather(g, ki, ci, nq, &m);
    if (nq.max_nn != 0 && n > nq.max_nn) {
      double last_d2;
      int32_t last_ix;
      normals_select(g, ki, ci, nq, list_d2.data(), list_ix.data(), 1, &last_d2, &last_ix);
      n = normals_gather_capped(g, ki, ci, nq, last_d2, last_ix, &m);
    }
    double C[6];
    normals_covariance(m, n, C);
    normals_finish(C, n, ci, false, 0.0, 0.0, 0.0, &normals[4 * v]);
    counts[v] = n;
  }

  // the records, the block maps of the levels and the trees' words: the host side of the call
  constexpr int kLevels = 3;
  std::vector<RegFrame> fr((size_t)F + 1);
  std::vector<int64_t> map((size_t)kLevels * (F + 1), 0);
  int64_t words = 0, live = 0;
  for (int64_t f = 0; f < F; ++f) {
    RegPose T;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) T.R[3 * r + k] = inits[16 * f + 4 * r + k];
      T.t[r] = inits[16 * f + 4 * r + 3];
    }
    if (!register_pose_ok(T)) return 4;
    words += register_frame_init(&fr[f], T, counts_f[f], words);
    int64_t cnt = fr[f].blocks;
    for (int l = 0; l < kLevels; ++l) {
      int64_t* off = map.data() + (size_t)l * (F + 1);
      off[f + 1] = off[f] + cnt;
      cnt = cnt >= kRegBlock ? cnt / kRegBlock : 0;
    }
    live += fr[f].status == kRegGoOn;
  }
  std::vector<double> tree((size_t)words + 1, 0.0), history((size_t)kRegHistory * F * max_iterations + 1, 0.0);

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  if (M) {
    std::fwrite(normals.data(), 8, (size_t)4 * M, out);
    std::fwrite(counts.data(), 4, (size_t)M, out);
  }
  const int64_t B = map[F];
  std::fwrite(&B, 8, 1, out);
  for (int64_t b = 0; b < B; ++b) {
    const int32_t f = register_block_frame(map.data(), (int32_t)F, b);
    if (f < 0 || f >= F || b < map[f] || b >= map[f + 1]) return 5;   // the block is inside its frame's span
    std::fwrite(&f, 4, 1, out);
  }

  NormalsQuery w;
  w.R = (int32_t)std::ceil(max_distance / h);
  if (w.R < 1) w.R = 1;
  w.max_nn = 0;
  w.r2 = max_distance * max_distance;
  static double x[kRegSums][kRegBlock];
  int64_t ran = 0;
  for (int32_t it = 0; live > 0 && it < max_iterations; ++it, ++ran) {
    // k_rg_frames_step
    for (int64_t b = 0; b < B; ++b) {
      const int32_t f = register_block_frame(map.data(), (int32_t)F, b);
      RegFrame& r = fr[f];
      if (r.status != kRegGoOn) continue;
      const int64_t lb = b - map[f];
      if (lb * kRegBlock >= r.n) continue;
      for (int t = 0; t < kRegBlock; ++t) {
        const int64_t i = lb * kRegBlock + t;
        double q[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
        bool pair = false;
        if (i < r.n) {
          register_move(r.T, &src[3 * (doff[f] + i)], q);
          int32_t id = -1;
          double d2;
          if (M > 0) register_nearest(g, h, o, w, q, &id, &d2);
          if (id >= 0 && counts[id] >= kNormalsMinNN) {
            for (int a = 0; a < 3; ++a) {
              c[a] = cent[(size_t)kNormalsCent * id + a];
              n[a] = normals[(size_t)4 * id + a];
            }
            pair = true;
          }
        }
        double leaf[kRegSums];
        register_leaf(pair, q, c, n, leaf);
        for (int k = 0; k < kRegSums; ++k) x[k][t] = leaf[k];
        r.count += pair;
      }
      block_tree(x, tree.data() + r.tree + lb, r.blocks);
    }
    // k_rg_frames_tree, level by level
    for (int l = 1; l < kLevels; ++l) {
      const int64_t* off = map.data() + (size_t)l * (F + 1);
      for (int64_t b = 0; b < off[F]; ++b) {
        const int32_t f = register_block_frame(off, (int32_t)F, b);
        const RegFrame& r = fr[f];
        if (r.status != kRegGoOn) continue;
        int64_t cnt;
        const int64_t from = register_level(r.blocks, l, &cnt);
        const double* lvl = tree.data() + r.tree + from;
        const int64_t lb = b - off[f];
        for (int k = 0; k < kRegSums; ++k)
          for (int t = 0; t < kRegBlock; ++t) x[k][t] = lvl[k * cnt + lb * kRegBlock + t];
        block_tree(x, tree.data() + r.tree + from + (int64_t)kRegSums * cnt + lb, cnt / kRegBlock);
      }
    }
    // k_rg_frames_solve
    live = 0;
    for (int64_t f = 0; f < F; ++f) {
      RegFrame& r = fr[f];
      if (r.status != kRegGoOn) continue;
      double top[kRegTopMax], sums[kRegSums];
      if (r.top_n < 1 || r.top_n > kRegTopMax) return 5;
      for (int k = 0; k < kRegSums; ++k) {
        for (int i = 0; i < r.top_n; ++i) top[i] = tree[r.top + (int64_t)k * r.top_n + i];
        sums[k] = register_tail(top, r.top_n);
      }
      live += register_frame_end(&r, sums, max_iterations, par[6], par[7], history.data() + (size_t)f * max_iterations * kRegHistory);
    }
  }
  for (int64_t f = 0; f < F; ++f) {
    const RegFrame& r = fr[f];
    const int64_t stats[4] = {r.pairs, r.iterations, r.status, r.n};
    double T[16] = {0};
    for (int a = 0; a < 3; ++a) {
      for (int k = 0; k < 3; ++k) T[4 * a + k] = r.T.R[3 * a + k];
      T[4 * a + 3] = r.T.t[a];
    }
    T[15] = 1.0;
    std::fwrite(stats, 8, 4, out);
    std::fwrite(T, 8, 16, out);
  }
  std::fwrite(history.data(), 8, (size_t)kRegHistory * F * max_iterations, out);
  std::fwrite(&ran, 8, 1, out);
  std::fclose(out);
  return 0;
}
