// normals.hpp — the kernels of the voxel cloud's surface normals (host side in voxel.hip; scalar core in
// normals_core.hpp).  They read the live voxel build: its key table, vid, vslot, sums and cnt.
//
// Three phases, one lane per voxel:
//   centroids   once per build: voxel_finalise's cx, cy, cz of every voxel into a dense array by voxel id
//               (32 B records), so a probe that hits costs key -> vid -> centroid, not the 36-byte record and
//               six conversions and divisions per neighbour
//   window      the (2R + 1)^3 probes of the voxel's window in key order, accumulating the moments while it
//               probes; a voxel with at most max_nn neighbours is finished here, with no storage.  One that
//               finds more is appended to the capped list (its place there does not reach the output)
//   cap         one lane per capped voxel, 64 lanes per workgroup: a second walk selects the max_nn smallest
//               (d2, key) through a per-lane list in LDS, a third accumulates those in key order
//
// Kept normals (mc_voxel_keep_normals): after an edit of the cloud only the rows of the dirty set are estimated again
//   mark        one lane per item of the edit (per voxel of a removal): claim, centroid, window marking
//   window      the window phase with the voxel taken from the dirty list; the cap phase follows as it is, its list
//               being one of voxel ids already
//   carry       a removal: the kept rows and counts of the survivors to their new ids, and the dirty list in new ids
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "normals_core.hpp"
#include "voxel.hpp"

namespace mc {

constexpr int kNrmCapBlock = 64;   // lanes per workgroup of the cap kernel: 64 * 64 * (8 + 2) B = 40 KB of LDS

struct NrmArgs {
  NormalsGrid g;
  const uint32_t* vslot;
  int64_t M;
  NormalsQuery q;
  double viewpoint[3];
  int32_t has_viewpoint;
  double* normals;     // (M, 4) nx, ny, nz, curvature; 16-byte aligned
  int32_t* counts;     // (M,) or null
  double* cov;         // (M, 6) or null; 16-byte aligned
  uint32_t* capped;    // M: the voxels the cap applies to
  uint32_t* n_capped;  // [0]
  const uint32_t* list;   // k_nrm_window<true>: the n_list voxels to estimate (a refresh of kept normals)
  int64_t n_list;
};

__global__ __launch_bounds__(kVoxBlock) void k_nrm_centroids(VoxOut a, double* cent) {
  const int64_t v = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.M) return;
  int32_t k[3];
  double out[4];
  int64_t n;
  vox_finalise_one(a, v, k, out, &n);
  double2* o = reinterpret_cast<double2*>(cent + kNormalsCent * v);
  o[0] = make_double2(out[0], out[1]);
  o[1] = make_double2(out[2], 0.0);
}

__device__ __forceinline__ void nrm_store(const NrmArgs& a, int64_t v, const NormalsMoments& m, int32_t n,
                                          const double ci[3]) {
  double C[6], out[4];
  normals_covariance(m, n, C);
  normals_finish(C, n, ci, a.has_viewpoint != 0, a.viewpoint[0], a.viewpoint[1], a.viewpoint[2], out);
  double2* o = reinterpret_cast<double2*>(a.normals + 4 * v);
  o[0] = make_double2(out[0], out[1]);
  o[1] = make_double2(out[2], out[3]);
  if (a.counts) a.counts[v] = n;
  if (a.cov) {
    double2* c = reinterpret_cast<double2*>(a.cov + 6 * v);
    c[0] = make_double2(C[0], C[1]);
    c[1] = make_double2(C[2], C[3]);
    c[2] = make_double2(C[4], C[5]);
  }
}

__device__ __forceinline__ void nrm_voxel(const NrmArgs& a, int64_t v, int32_t ki[3], double ci[3]) {
  voxel_unpack(a.g.keys[a.vslot[v]], ki);
  const double* c = a.g.cent + kNormalsCent * v;
  ci[0] = c[0];
  ci[1] = c[1];
  ci[2] = c[2];
}

// kList: lane i takes voxel list[i] of n_list (the capped list holds at most n_list then); else voxel i of M
template <bool kList>
__global__ __launch_bounds__(kVoxBlock) void k_nrm_window(NrmArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (i >= (kList ? a.n_list : a.M)) return;
  const int64_t v = kList ? (int64_t)a.list[i] : i;
  int32_t ki[3];
  double ci[3];
  nrm_voxel(a, v, ki, ci);
  NormalsMoments m;
  const int32_t found = normals_gather(a.g, ki, ci, a.q, &m);
  if (a.q.max_nn != 0 && found > a.q.max_nn) {
    a.capped[atomicAdd(a.n_capped, 1u)] = (uint32_t)v;   // fewer than M appends: inside the list
    return;
  }
  nrm_store(a, v, m, found, ci);
}

__global__ __launch_bounds__(kNrmCapBlock) void k_nrm_cap(NrmArgs a) {
  __shared__ double list_d2[kNormalsMaxNN * kNrmCapBlock];
  __shared__ uint16_t list_ix[kNormalsMaxNN * kNrmCapBlock];
  const int64_t i = (int64_t)blockIdx.x * kNrmCapBlock + threadIdx.x;
  if (i >= (int64_t)*a.n_capped) return;
  const int64_t v = a.capped[i];
  int32_t ki[3];
  double ci[3];
  nrm_voxel(a, v, ki, ci);
  // entry e of lane l at [e * 64 + l]: max_nn <= kNormalsMaxNN entries, so inside both arrays
  double last_d2;
  int32_t last_ix;
  normals_select(a.g, ki, ci, a.q, list_d2 + threadIdx.x, list_ix + threadIdx.x, kNrmCapBlock, &last_d2, &last_ix);
  NormalsMoments m;
  const int32_t kept = normals_gather_capped(a.g, ki, ci, a.q, last_d2, last_ix, &m);
  nrm_store(a, v, m, kept, ci);
}

// ---- kept normals: what an edit makes stale (normals_core.hpp "kept normals") -------------------------------------------
// the stamps of the voxels on the device: a lane that reads the epoch has nothing to claim (stamps reach the epoch
// only inside this edit), so many items of one voxel send one exchange each at the most, and mostly none
struct NrmStamps {
  uint32_t* w;
  __device__ __forceinline__ uint32_t exchange(uint32_t v, uint32_t epoch) {
    if (__hip_atomic_load(w + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) return epoch;
    return atomicExch(w + v, epoch);
  }
};

struct NrmMarkArgs {
  NormalsGrid g;           // the table after the edit's records are in (before a removal's refill); cent is not read
  VoxOut rec;              // the records, for the centroids of the touched voxels
  const uint32_t* slot;    // items: the slot of every item's voxel
  const uint8_t* keep;     // a removal: the keep byte of every voxel
  int64_t n;               // items, or the voxels of a removal
  int32_t R;
  uint32_t epoch;
  uint32_t* touched;       // stamps: the voxels an item of this edit landed in
  uint32_t* dirty;         // stamps: the voxels whose window holds a touched cell
  uint32_t* list;          // items: the dirty voxels, each once, in no order
  uint32_t* n_list;        // [0]
  double* cent;            // by voxel id
};

// kRemoval false: one lane per item.  The first lane of a voxel rewrites its centroid (one that still holds points)
// and walks its window, appending every voxel it is first to claim to the list; no lane waits for another.
// kRemoval true: one lane per voxel of the cloud; a removed one walks its window and stamps what it finds, and the
// list is made of the survivors' stamps afterwards (k_nrm_carry), under their new ids
template <bool kRemoval>
__global__ __launch_bounds__(kVoxBlock) void k_nrm_mark(NrmMarkArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (i >= a.n) return;
  NrmStamps dirty = {a.dirty};
  int32_t ki[3];
  if (kRemoval) {
    if (a.keep[i]) return;
    voxel_unpack(a.g.keys[a.rec.vslot[i]], ki);
    normals_mark_window(a.g, ki, a.R, a.epoch, dirty, [](uint32_t) {});
    return;
  }
  const uint32_t at = a.slot[i];
  if (at == kVoxNone) return;
  const uint32_t v = a.g.vid[at];
  NrmStamps touched = {a.touched};
  if (!normals_claim(touched, v, a.epoch)) return;
  if (a.rec.cnt[v] != 0) {   // a voxel a subtraction emptied leaves with the call: it has no centroid
    double out[4];
    int64_t n;
    vox_finalise_one(a.rec, v, ki, out, &n);
    double2* o = reinterpret_cast<double2*>(a.cent + kNormalsCent * (int64_t)v);
    o[0] = make_double2(out[0], out[1]);
    o[1] = make_double2(out[2], 0.0);
  } else {
    voxel_unpack(a.g.keys[at], ki);
  }
  normals_mark_window(a.g, ki, a.R, a.epoch, dirty, [&](uint32_t u) {
    a.list[atomicAdd(a.n_list, 1u)] = u;   // a voxel is claimed once: fewer than M appends
  });
}

struct NrmCarryArgs {
  const uint32_t* ids;     // the M_keep survivors' old ids, ascending
  int64_t M_keep;
  const double* normals;   // the kept rows by old id
  const int32_t* counts;
  const uint32_t* dirty;   // the stamps by old id
  uint32_t epoch;
  double* normals_out;     // by new id
  int32_t* counts_out;
  uint32_t* list;          // the new ids of the survivors stamped in this edit
  uint32_t* n_list;
};

// one lane per survivor: its kept row and count to its new id; a stamped one is listed for the refresh
__global__ __launch_bounds__(kVoxBlock) void k_nrm_carry(NrmCarryArgs a) {
  const int64_t j = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (j >= a.M_keep) return;
  const int64_t v = a.ids[j];
  const double2* r = reinterpret_cast<const double2*>(a.normals + 4 * v);
  const double2 lo = r[0], hi = r[1];
  double2* w = reinterpret_cast<double2*>(a.normals_out + 4 * j);
  w[0] = lo;
  w[1] = hi;
  a.counts_out[j] = a.counts[v];
  if (a.dirty[v] == a.epoch) a.list[atomicAdd(a.n_list, 1u)] = (uint32_t)j;
}

}  // namespace mc
