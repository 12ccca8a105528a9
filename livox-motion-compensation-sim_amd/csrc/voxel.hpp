// voxel.hpp — the kernels of the voxel-grid filter (voxel.hip; scalar core in voxel_core.hpp).
//
// A point's index p is its place in the source: the row for float64 rows, frame-major then the index
// within the frame for a batch (padding slots are not points).  Four phases, no sort:
//   insert      every point's key into an open-addressing table (capacity a power of two >= 2 N):
//               atomicCAS on the 8-byte key, atomicMin of p on the slot's "first index"; the point's
//               slot is kept (4 bytes per point), so no later phase probes again
//   rank        flag[p] = (first[slot[p]] == p); the flags' exclusive scan is the voxel's place in the
//               output (order of first appearance) — a function of indices alone, so deterministic
//   accumulate  per point 64-bit integer atomic adds of Q[3] and QI and a 32-bit add of 1 into the
//               voxel's record: integer sums do not depend on the order the atomics arrive in
//   finalise    one lane per voxel (four voxels per lane into a batch), 16-byte stores
//
// Growing a live cloud (mc_voxel_insert_*, mc_voxel_merge_sums).  An item is a point, or a voxel record (key, n,
// S[3], SI) standing for n points of that voxel arriving together; its index p is its place in the call's source.
// Between calls the table holds this invariant, which the build leaves and every insert restores:
//   keys[slot]   kVoxelEmpty, or the key of voxel vid[slot], with vslot[vid[slot]] == slot
//   first[slot]  kVoxNone in an empty slot, a value below kVoxNewBit in an occupied one
// so an insert tells a voxel of the cloud (first < kVoxNewBit) from a key of its own call (first >= kVoxNewBit)
// without a pass over the table, and its cost is that of its items:
//   validate    every item quantised or checked, atomicMin of a refused p; the table is not touched before the
//               host has seen that none is refused, so a refused call changes nothing
//   grow        M + items > cap / 2 (voxel_table_log2): a fresh table, one lane per voxel re-inserts the key it
//               finds through vslot (keys are distinct: CAS alone) and writes vid, first and the new vslot
//   insert      the build's probe; a lane that ends in a slot with first >= kVoxNewBit takes part in the
//               atomicMin of kVoxNewBit | p, a lane at a voxel of the cloud leaves first alone
//   rank        the build's flag / scan / rank over the call's items: flag[p] = (first[slot[p]] == kVoxNewBit | p);
//               the new voxels are M_old + rank, and the flagged lane puts first[slot] below kVoxNewBit again
//   accumulate  as the build's, a record adding its sums and its n
//
// Taking voxels and points out (mc_voxel_remove, mc_voxel_subtract_*).  A removal keeps the survivors' order and
// gives them ids 0 .. M' - 1; it leaves the invariant above as a growth does, the first index of every survivor 0:
//   keep        a keep byte per voxel (not mask[v], or cnt[v] != 0), and the ascending survivor ids by the flag /
//               scan / scatter of the selection (plane.hpp)
//   compact     one lane per survivor j of old id v: the 32-byte record and the count into fresh arrays at j (a
//               stable compaction in place is not safe in parallel; the arrays are swapped afterwards), its packed
//               key, found through vslot, into an 8-byte scratch at j; the points of the survivors into one word
//   refill      the table cleared (shrunk when the survivors fill less than an eighth of it, voxel_table_shrink_log2)
//               and filled from the scratch as a growth fills its new one: CAS alone, vid = j, first = 0, vslot[j]
// so its cost is that of the cloud, not of what leaves.  A subtraction costs what its items cost unless a voxel
// empties, which ends in the removal of the voxels with cnt == 0:
//   validate    every item quantised or checked and its key looked up, read-only: atomicMin of the lowest item the
//               filter refuses (meta[0]) and of the lowest whose voxel the cloud lacks (meta[1]); slot[p] kept
//   apply       the accumulate with the opposite sign; the count is a uint32 that a subtraction of more than it
//               holds leaves at 2^31 or above (a call brings at most N < 2^31 points), read as negative
//   check       per item its voxel's record against voxel_remainder_ok: atomicMin of the lowest item that fails
//               (meta[0]), a flag where a count is 0 (meta[1]); on a failure apply runs again with the sign of an
//               insert, which restores every record exactly
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.hpp"
#include "voxel_core.hpp"

namespace mc {

constexpr int kVoxBlock = 256;          // threads per workgroup
constexpr int kVoxPerThread = 8;        // points per thread of the rank kernels
constexpr int kVoxChunk = kVoxBlock * kVoxPerThread;   // points per workgroup of the rank kernels
constexpr uint32_t kVoxNone = kVoxelNoSlot;   // no slot (a refused point) / no first index yet
constexpr uint32_t kVoxNewBit = 0x80000000u;  // first[slot] of a key the running insert created: kVoxNewBit | lowest p
enum VoxKind { kVoxRows = 0, kVoxBatch = 1, kVoxRecords = 2 };   // the source of an insert

typedef float vox_f4 __attribute__((ext_vector_type(4)));

struct VoxSrc {
  // a batch: blocked columns (layout.hpp), frames on 256-point blocks
  const float* cols;
  int32_t C, F;
  const int64_t* poff;     // F + 1 padded offsets
  const int64_t* doff;     // F + 1 dense offsets
  const int64_t* counts;   // F
  int64_t P;               // padded points (a multiple of 256)
  // float64 rows x, y, z, intensity, ...
  const double* rows;
  int64_t ld;
  int64_t n;               // points
  double h, o[3];
};

// voxel records as the source of a merge
struct VoxRecSrc {
  const int32_t* keys;     // (n, 3)
  const int32_t* counts;   // (n,)
  const long long* sums;   // (n, 4) = Sx, Sy, Sz, SI
  int64_t n;
};

struct VoxTable {
  unsigned long long* keys;   // cap
  uint32_t* first;            // cap: the lowest p of the slot's key
  uint32_t* vid;              // cap: the voxel's place in the output (rank phase)
  uint32_t* slot;             // n: the point's slot (kVoxNone: refused)
  int shift;                  // 64 - log2(cap)
  uint32_t mask;              // cap - 1
  uint32_t* meta;             // [0] lowest refused p (kVoxNone: none), [1] M, [2..3] an insert's points (64 bits)
};

// the points of one lane: BATCH, the float4 group g of the padded columns (4 points of one frame);
// else row g.  fn(p, v, intensity) for each real point.
template <bool BATCH, typename Fn>
__device__ __forceinline__ void vox_points(const VoxSrc& s, int64_t g, Fn&& fn) {
  if (BATCH) {
    const int64_t pp = g * 4;
    if (pp >= s.P) return;
    // the wave's 64 groups are one 256-point block: its frame is wave-uniform
    const int64_t blk0 = (int64_t)__builtin_amdgcn_readfirstlane((int)(pp >> 8)) << 8;
    int32_t lo = 0, hi = s.F - 1;
    while (lo < hi) {   // the first frame whose padded end is beyond the block
      const int32_t mid = (lo + hi) >> 1;
      if (ldu(s.poff + mid + 1) <= blk0) lo = mid + 1;
      else hi = mid;
    }
    const int64_t local = pp - ldu(s.poff + lo), cnt = ldu(s.counts + lo), d0 = ldu(s.doff + lo) + local;
    if (local >= cnt) return;
    const float* b = s.cols + bidx(s.C, 0, pp);
    const vox_f4 x = __builtin_nontemporal_load(reinterpret_cast<const vox_f4*>(b));
    const vox_f4 y = __builtin_nontemporal_load(reinterpret_cast<const vox_f4*>(b + kBlkPts));
    const vox_f4 z = __builtin_nontemporal_load(reinterpret_cast<const vox_f4*>(b + 2 * kBlkPts));
    const vox_f4 w = __builtin_nontemporal_load(reinterpret_cast<const vox_f4*>(b + 3 * kBlkPts));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (local + j < cnt) {
        const double v[3] = {(double)x[j], (double)y[j], (double)z[j]};
        fn(d0 + j, v, (double)w[j]);
      }
    }
  } else {
    if (g >= s.n) return;
    const double* r = s.rows + g * s.ld;
    const double v[3] = {__builtin_nontemporal_load(r), __builtin_nontemporal_load(r + 1),
                         __builtin_nontemporal_load(r + 2)};
    fn(g, v, __builtin_nontemporal_load(r + 3));
  }
}

template <bool BATCH>
__global__ __launch_bounds__(kVoxBlock) void k_vox_insert(VoxSrc s, VoxTable t) {
  const int64_t g = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  vox_points<BATCH>(s, g, [&](int64_t p, const double v[3], double inten) {
    const VoxelPoint q = voxel_quantise(v, inten, s.h, s.o);
    if (q.bad) {
      atomicMin(t.meta, (uint32_t)p);
      t.slot[p] = kVoxNone;
      return;
    }
    const unsigned long long key = voxel_pack(q.k);
    uint32_t at = voxel_slot_first(key, t.shift, t.mask);
    // the table is at most half full, so a probe ends; a key, once written, never changes, so a plain
    // (device-coherent) load that sees it saves the CAS.  The probe never yields slot kVoxelNoSlot
    // (= kVoxNone, reachable only in a table of 2^32 slots), so slot[p] == kVoxNone means refused.
    for (;;) {
      unsigned long long cur = __hip_atomic_load(t.keys + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kVoxelEmpty) cur = atomicCAS(t.keys + at, (unsigned long long)kVoxelEmpty, key);
      if (cur == kVoxelEmpty || cur == key) break;
      at = voxel_slot_next(at, t.mask);
    }
    atomicMin(t.first + at, (uint32_t)p);
    t.slot[p] = at;
  });
}

// the workgroup's sum of v (every thread takes part), in every thread; *excl: the sum of the threads before
__device__ __forceinline__ uint32_t vox_block_scan(uint32_t v, uint32_t* excl) {
  __shared__ uint32_t wave_tot[kVoxBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  __syncthreads();   // wave_tot may still be read from a previous call
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kVoxBlock / 64; ++w) {
    const uint32_t tw = wave_tot[w];
    if (w < wave) before += tw;
    total += tw;
  }
  *excl = before + inc - v;
  return total;
}

// flags of the chunk's points (bit j of byte t: point chunk * kVoxChunk + 8 t + j is the first of its
// voxel) and the chunk's count.  LIVE: of an insert, whose first indices carry kVoxNewBit
template <bool LIVE>
__global__ __launch_bounds__(kVoxBlock) void k_vox_flag(VoxTable t, int64_t n, uint8_t* flags, uint32_t* chunk_count) {
  const int64_t base = ((int64_t)blockIdx.x * kVoxBlock + threadIdx.x) * kVoxPerThread;
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < kVoxPerThread; ++j) {
    const int64_t p = base + j;
    if (p < n) {
      const uint32_t at = t.slot[p];
      if (at != kVoxNone && t.first[at] == (LIVE ? kVoxNewBit | (uint32_t)p : (uint32_t)p)) bits |= 1u << j;
    }
  }
  flags[(int64_t)blockIdx.x * kVoxBlock + threadIdx.x] = (uint8_t)bits;
  uint32_t excl;
  const uint32_t total = vox_block_scan(__builtin_popcount(bits), &excl);
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// exclusive scan of the chunk counts, in place, by one workgroup; the total (M) to meta[1]
__global__ __launch_bounds__(kVoxBlock) void k_vox_scan(uint32_t* chunk_count, int64_t n_chunks, uint32_t* meta) {
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < n_chunks; b0 += kVoxBlock) {
    const int64_t i = b0 + threadIdx.x;
    const uint32_t v = i < n_chunks ? chunk_count[i] : 0u;
    uint32_t excl;
    const uint32_t total = vox_block_scan(v, &excl);
    if (i < n_chunks) chunk_count[i] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) meta[1] = carry;
}

// vid[slot] and vslot[rank] of every flagged point.  LIVE: ranks follow the cloud's `base` voxels, and the slot's
// first index goes back below kVoxNewBit (the table's invariant between calls)
template <bool LIVE>
__global__ __launch_bounds__(kVoxBlock) void k_vox_rank(VoxTable t, int64_t n, const uint8_t* flags,
                                                        const uint32_t* chunk_off, uint32_t* vslot, uint32_t base_rank) {
  const int64_t base = ((int64_t)blockIdx.x * kVoxBlock + threadIdx.x) * kVoxPerThread;
  const uint32_t bits = flags[(int64_t)blockIdx.x * kVoxBlock + threadIdx.x];
  uint32_t excl;
  vox_block_scan(__builtin_popcount(bits), &excl);
  uint32_t rank = (LIVE ? base_rank : 0u) + chunk_off[blockIdx.x] + excl;
#pragma unroll
  for (int j = 0; j < kVoxPerThread; ++j) {
    if (bits & (1u << j)) {   // a set bit has p < n and a slot
      const uint32_t at = t.slot[base + j];
      t.vid[at] = rank;
      vslot[rank] = at;
      if (LIVE) t.first[at] = (uint32_t)(base + j);
      ++rank;
    }
  }
}

// a voxel's record: 4 int64 words in sums (S[3], SI) and its count in cnt (a 64-byte record with the
// count inside measured 4-13 % slower)
constexpr int kVoxRec = 4;

template <bool BATCH>
__global__ __launch_bounds__(kVoxBlock) void k_vox_accumulate(VoxSrc s, VoxTable t, long long* sums, uint32_t* cnt) {
  const int64_t g = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  vox_points<BATCH>(s, g, [&](int64_t p, const double v[3], double inten) {
    const uint32_t at = t.slot[p];
    if (at == kVoxNone) return;
    const VoxelPoint q = voxel_quantise(v, inten, s.h, s.o);
    const int64_t vox = t.vid[at];
    long long* r = sums + kVoxRec * vox;
    (void)__hip_atomic_fetch_add(r + 0, (long long)q.Q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 1, (long long)q.Q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 2, (long long)q.Q[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 3, (long long)q.QI, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(cnt + vox, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
}

// ---- growing a live cloud ---------------------------------------------------------------------------------------------
// the items of one lane: fn(p, q, n) with q the point quantised (n = 1) or the record as a VoxelPoint (Q = S, QI = SI,
// bad: refused by voxel_record_ok)
template <int KIND, typename Src, typename Fn>
__device__ __forceinline__ void vox_items(const Src& s, int64_t g, Fn&& fn) {
  if constexpr (KIND == kVoxRecords) {
    if (g >= s.n) return;
    VoxelPoint q;
    const int64_t n = s.counts[g];
    const long long* r = s.sums + 4 * g;
    for (int c = 0; c < 3; ++c) {
      q.k[c] = s.keys[3 * g + c];
      q.Q[c] = r[c];
    }
    q.QI = r[3];
    q.bad = voxel_record_ok(q.k, n, q.Q, q.QI) ? 0 : 1;
    fn(g, q, (uint32_t)n);
  } else {
    vox_points<KIND == kVoxBatch>(s, g, [&](int64_t p, const double v[3], double inten) {
      fn(p, voxel_quantise(v, inten, s.h, s.o), 1u);
    });
  }
}

// meta[0] = the lowest refused item (kVoxNone: none); records: meta[2..3] += the points of the accepted ones.
// Points: a lane per group, as the other phases.  Records: a workgroup per chunk of kVoxChunk, so the one word that
// takes the sum sees one add per 2048 records (a single word takes ~88 atomics per microsecond, MI355X_MICROARCH.md
// "dequeue": one add per wave was 10 ms for 59 M records).
template <int KIND, typename Src>
__global__ __launch_bounds__(kVoxBlock) void k_vox_validate(Src s, uint32_t* meta) {
  constexpr int kPer = KIND == kVoxRecords ? kVoxPerThread : 1;
  unsigned long long pts = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t g = ((int64_t)blockIdx.x * kPer + j) * kVoxBlock + threadIdx.x;
    vox_items<KIND>(s, g, [&](int64_t p, const VoxelPoint& q, uint32_t n) {
      if (q.bad) atomicMin(meta, (uint32_t)p);
      else pts += n;
    });
  }
  if constexpr (KIND == kVoxRecords) {   // every thread of the workgroup is here
    __shared__ unsigned long long wave_pts[kVoxBlock / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pts += __shfl_xor(pts, d, 64);
    if ((threadIdx.x & 63) == 0) wave_pts[threadIdx.x >> 6] = pts;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < kVoxBlock / 64; ++w) total += wave_pts[w];
      if (total) atomicAdd(reinterpret_cast<unsigned long long*>(meta + 2), total);
    }
  }
}

// one lane per voxel of the cloud: its key out of the old table into the new one (t), keys being distinct
__global__ __launch_bounds__(kVoxBlock) void k_vox_rehash(const unsigned long long* old_keys, uint32_t* vslot, int64_t M,
                                                          VoxTable t) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= M) return;
  const unsigned long long key = old_keys[vslot[v]];
  uint32_t at = voxel_slot_first(key, t.shift, t.mask);
  while (atomicCAS(t.keys + at, (unsigned long long)kVoxelEmpty, key) != kVoxelEmpty) at = voxel_slot_next(at, t.mask);
  t.vid[at] = (uint32_t)v;
  t.first[at] = 0u;
  vslot[v] = at;
}

// k_vox_insert into a table that holds a cloud (the header's invariant); the call's items have passed k_vox_validate
template <int KIND, typename Src>
__global__ __launch_bounds__(kVoxBlock) void k_vox_insert_live(Src s, VoxTable t) {
  const int64_t g = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  vox_items<KIND>(s, g, [&](int64_t p, const VoxelPoint& q, uint32_t) {
    if (q.bad) {
      t.slot[p] = kVoxNone;
      return;
    }
    const unsigned long long key = voxel_pack(q.k);
    uint32_t at = voxel_slot_first(key, t.shift, t.mask);
    for (;;) {   // as k_vox_insert
      unsigned long long cur = __hip_atomic_load(t.keys + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kVoxelEmpty) cur = atomicCAS(t.keys + at, (unsigned long long)kVoxelEmpty, key);
      if (cur == kVoxelEmpty || cur == key) break;
      at = voxel_slot_next(at, t.mask);
    }
    // a voxel of the cloud keeps its first index below kVoxNewBit through the whole call, a key of this call
    // never gets below it: whichever value the load sees decides the same
    if (__hip_atomic_load(t.first + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= kVoxNewBit)
      atomicMin(t.first + at, kVoxNewBit | (uint32_t)p);
    t.slot[p] = at;
  });
}

template <int KIND, typename Src>
__global__ __launch_bounds__(kVoxBlock) void k_vox_accumulate_items(Src s, VoxTable t, long long* sums, uint32_t* cnt) {
  const int64_t g = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  vox_items<KIND>(s, g, [&](int64_t p, const VoxelPoint& q, uint32_t n) {
    const uint32_t at = t.slot[p];
    if (at == kVoxNone) return;
    const int64_t vox = t.vid[at];
    long long* r = sums + kVoxRec * vox;
    (void)__hip_atomic_fetch_add(r + 0, (long long)q.Q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 1, (long long)q.Q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 2, (long long)q.Q[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 3, (long long)q.QI, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(cnt + vox, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
}

// ---- taking voxels and points out ---------------------------------------------------------------------------------------
typedef long long vox_l2 __attribute__((ext_vector_type(2)));

// *w = min(*w, p).  The word only falls, so a lane whose p is not below what it reads has nothing to add: a call
// in which many items fail sends few atomics to the one word (~88 per microsecond, MI355X_MICROARCH.md "dequeue")
__device__ __forceinline__ void vox_lowest(uint32_t* w, int64_t p) {
  if ((uint32_t)p < __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(w, (uint32_t)p);
}

// *word += the workgroup's sum of v, one add per workgroup (every thread takes part)
__device__ __forceinline__ void vox_block_add(unsigned long long v, unsigned long long* word) {
  __shared__ unsigned long long wave_sum[kVoxBlock / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kVoxBlock / 64; ++w) total += wave_sum[w];
    if (total) atomicAdd(word, total);
  }
}

// the keep byte of every voxel.  MASK: its mask byte is clear (mc_voxel_remove); else: its count is not 0
template <bool MASK>
__global__ __launch_bounds__(kVoxBlock) void k_vox_keep(const uint8_t* mask, const uint32_t* cnt, int64_t M, uint8_t* keep) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= M) return;
  keep[v] = MASK ? (mask[v] == 0 ? 1 : 0) : (cnt[v] != 0 ? 1 : 0);
}

struct VoxCompact {
  const uint32_t* ids;               // the M_keep survivors' old ids, ascending
  int64_t M_keep;
  const unsigned long long* keys;    // the table as it is
  const uint32_t* vslot;
  const long long* sums;
  const uint32_t* cnt;
  long long* sums_out;               // M_keep records (16-byte aligned, as sums)
  uint32_t* cnt_out;
  unsigned long long* keys_out;      // M_keep packed keys
  unsigned long long* points;        // += the survivors' points
};

// one lane per survivor: its record as two 16-byte words, its count and its key to place j
__global__ __launch_bounds__(kVoxBlock) void k_vox_compact(VoxCompact a) {
  const int64_t j = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  unsigned long long pts = 0;
  if (j < a.M_keep) {
    const int64_t v = a.ids[j];
    const vox_l2* r = reinterpret_cast<const vox_l2*>(a.sums + kVoxRec * v);
    const vox_l2 lo = r[0], hi = r[1];
    vox_l2* w = reinterpret_cast<vox_l2*>(a.sums_out + kVoxRec * j);
    w[0] = lo;
    w[1] = hi;
    const uint32_t n = a.cnt[v];
    a.cnt_out[j] = n;
    a.keys_out[j] = a.keys[a.vslot[v]];
    pts = n;
  }
  vox_block_add(pts, a.points);
}

// one lane per voxel of the compacted cloud: its key out of the scratch into the cleared table t, as k_vox_rehash
__global__ __launch_bounds__(kVoxBlock) void k_vox_refill(const unsigned long long* keys_in, uint32_t* vslot, int64_t M, VoxTable t) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= M) return;
  const unsigned long long key = keys_in[v];
  uint32_t at = voxel_slot_first(key, t.shift, t.mask);
  while (atomicCAS(t.keys + at, (unsigned long long)kVoxelEmpty, key) != kVoxelEmpty) at = voxel_slot_next(at, t.mask);
  t.vid[at] = (uint32_t)v;
  t.first[at] = 0u;
  vslot[v] = at;
}

// meta[0] = the lowest item the filter refuses, meta[1] = the lowest whose voxel the cloud does not hold (kVoxNone:
// none); slot[p] = the slot of the item's voxel; records: meta[2..3] += the points of the items found, as
// k_vox_validate adds them.  The table (t.keys null: a cloud without one) is read and not written
template <int KIND, typename Src>
__global__ __launch_bounds__(kVoxBlock) void k_vox_sub_validate(Src s, VoxTable t, uint32_t* meta) {
  constexpr int kPer = KIND == kVoxRecords ? kVoxPerThread : 1;
  unsigned long long pts = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t g = ((int64_t)blockIdx.x * kPer + j) * kVoxBlock + threadIdx.x;
    vox_items<KIND>(s, g, [&](int64_t p, const VoxelPoint& q, uint32_t n) {
      if (q.bad) {
        vox_lowest(meta, p);
        t.slot[p] = kVoxNone;
        return;
      }
      uint32_t at = kVoxNone;
      if (t.keys) {   // at most half full, so the probe ends at the key or at an empty slot
        const unsigned long long key = voxel_pack(q.k);
        at = voxel_slot_first(key, t.shift, t.mask);
        for (;;) {
          const unsigned long long cur = t.keys[at];
          if (cur == key) break;
          if (cur == kVoxelEmpty) { at = kVoxNone; break; }
          at = voxel_slot_next(at, t.mask);
        }
      }
      if (at == kVoxNone) vox_lowest(meta + 1, p);
      else pts += n;
      t.slot[p] = at;
    });
  }
  if constexpr (KIND == kVoxRecords) vox_block_add(pts, reinterpret_cast<unsigned long long*>(meta + 2));
}

// k_vox_accumulate_items times sign (-1: the items leave; +1: a refused call's items come back)
template <int KIND, typename Src>
__global__ __launch_bounds__(kVoxBlock) void k_vox_sub_apply(Src s, VoxTable t, long long* sums, uint32_t* cnt, int sign) {
  const int64_t g = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  vox_items<KIND>(s, g, [&](int64_t p, const VoxelPoint& q, uint32_t n) {
    const uint32_t at = t.slot[p];
    if (at == kVoxNone) return;
    const int64_t vox = t.vid[at];
    const long long sg = sign;
    long long* r = sums + kVoxRec * vox;
    (void)__hip_atomic_fetch_add(r + 0, sg * (long long)q.Q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 1, sg * (long long)q.Q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 2, sg * (long long)q.Q[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(r + 3, sg * (long long)q.QI, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(cnt + vox, sign < 0 ? 0u - n : n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
}

// one lane per item p < n: meta[0] = the lowest item whose voxel's record is no set of points any more, meta[1] = 1
// where a voxel is left without points
__global__ __launch_bounds__(kVoxBlock) void k_vox_sub_check(VoxTable t, int64_t n, const long long* sums, const uint32_t* cnt,
                                                             uint32_t* meta) {
  const int64_t p = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t at = t.slot[p];
  if (at == kVoxNone) return;
  const int64_t vox = t.vid[at];
  const long long* r = sums + kVoxRec * vox;
  const int64_t S[3] = {r[0], r[1], r[2]};
  const int64_t left = (int64_t)(int32_t)cnt[vox];   // below zero: more points taken than the voxel held
  if (!voxel_remainder_ok(left, S, r[3])) vox_lowest(meta, p);
  else if (left == 0 && __hip_atomic_load(meta + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
    __hip_atomic_store(meta + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct VoxOut {
  const unsigned long long* keys;
  const uint32_t* vslot;
  const long long* sums;
  const uint32_t* cnt;
  int64_t M;
  double h, o[3];
  double* rows;      // (M, 4) float64, 16-byte aligned, or null
  int32_t* counts;   // (M,) or null
  int32_t* keys_out; // (M, 3) or null
  float* cols;       // a one-frame batch of M points (C columns per block), or null
  int32_t C;
};

__device__ __forceinline__ void vox_finalise_one(const VoxOut& a, int64_t v, int32_t k[3], double out[4], int64_t* n) {
  voxel_unpack(a.keys[a.vslot[v]], k);
  const long long* r = a.sums + kVoxRec * v;
  const int64_t S[3] = {r[0], r[1], r[2]};
  *n = a.cnt[v];
  voxel_finalise(k, S, r[3], *n, a.h, a.o, out);
}

__global__ __launch_bounds__(kVoxBlock) void k_vox_emit_rows(VoxOut a) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  int32_t k[3];
  double out[4];
  int64_t n;
  vox_finalise_one(a, v, k, out, &n);
  if (a.rows) {
    double2* o = reinterpret_cast<double2*>(a.rows + 4 * v);
    o[0] = make_double2(out[0], out[1]);
    o[1] = make_double2(out[2], out[3]);
  }
  if (a.counts) a.counts[v] = (int32_t)n;
  if (a.keys_out) {
    a.keys_out[3 * v] = k[0];
    a.keys_out[3 * v + 1] = k[1];
    a.keys_out[3 * v + 2] = k[2];
  }
}

// four points per lane: one float4 per column of the out batch's single frame; point p < n is voxel voxel_of(p),
// the padding slots from n on get 0
template <typename VoxelOf>
__device__ __forceinline__ void vox_emit_four(const VoxOut& a, int64_t p0, int64_t n, VoxelOf&& voxel_of) {
  vox_f4 col[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p0 + j < n) {
      int32_t k[3];
      double out[4];
      int64_t cnt;
      vox_finalise_one(a, voxel_of(p0 + j), k, out, &cnt);
#pragma unroll
      for (int c = 0; c < 4; ++c) col[c][j] = (float)out[c];
    }
  }
  float* b = a.cols + bidx(a.C, 0, p0);
#pragma unroll
  for (int c = 0; c < 4; ++c) *reinterpret_cast<vox_f4*>(b + c * kBlkPts) = col[c];
}

// the whole cloud: point p is voxel p
__global__ __launch_bounds__(kVoxBlock) void k_vox_emit_batch(VoxOut a, int64_t P) {
  const int64_t p0 = ((int64_t)blockIdx.x * kVoxBlock + threadIdx.x) * 4;
  if (p0 >= P) return;
  vox_emit_four(a, p0, a.M, [](int64_t p) { return p; });
}

}  // namespace mc
