// voxel.hip — host side of the voxel-grid filter (include/mcdeskew.h mc_voxel_*; kernels in voxel.hpp).
//
// The filter's state (the key table, the per-point slots, the per-voxel sums and what the last build
// left for its emits) is the CtxExt in the context's voxel slot (internal.hpp): the other translation
// units see only that hook.  mc_voxel_release frees it early; mc_destroy frees what is left.  The surface
// normals of the built cloud (mc_voxel_normals; kernels in normals.hpp) and its density clustering
// (mc_voxel_clusters; kernels in cluster.hpp) read that state and keep theirs in it; so do its plane segmentation
// and the selection of a subset into a batch (mc_voxel_plane, mc_voxel_emit_selected; kernels in plane.hpp), and the
// registration of a source against the cloud (mc_voxel_nearest_*, mc_voxel_register_*, and every frame of a batch
// on its own in one call, mc_voxel_register_frames; kernels in register.hpp), and the walk of a scan's rays through the
// cloud (mc_voxel_rays_*; kernel in rays.hpp).
#include "../../include/mcdeskew.h"
#include "voxel.hpp"
#include "normals.hpp"
#include "cluster.hpp"
#include "plane.hpp"
#include "register.hpp"
#include "rays.hpp"
#include "internal.hpp"
#include "hostutil.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

using namespace mc;

namespace {

// Every timed phase of the unit, one line per stage.  A stage's mc_timing_read_* reads its line: {first, count}, the
// public phase index being the offset from `first`.  A new stage adds its line here and its range below, and nothing
// else: the state's one array of pairs is recycled, destroyed and read by these alone.
enum {
  kInsert, kRank, kAccumulate, kFinalise,
  kNrmCentroids, kNrmWindow, kNrmCap,
  kClDensity, kClUnion, kClLabel, kClNumber, kClStats,
  kPlCompact, kPlSample, kPlScore, kPlMask, kPlMoments, kPlSelect,
  kRgNormals, kRgCorrespond, kRgLeaves, kRgTree,   // the register's fifth phase, the solve, is the host's: no events
  kRfNormals, kRfStep, kRfTree, kRfSolve,
  kInsValidate, kInsInsert, kInsRank, kInsAccumulate,   // growing the live cloud; the insert's phase holds the table's growth
  kRmValidate, kRmApply, kRmCheck, kRmCompact,          // shrinking it; the compact phase holds the keep flags and the table's refill
  kRyClear, kRyWalk,                                    // the rays through it
  kKnMark, kKnWindow, kKnCap, kKnCarry,                 // the refresh of kept normals after an edit
  kAllPhases
};
struct PhaseRange { int first, count; };
constexpr PhaseRange kFilterPhases = {kInsert, 4}, kNormalsPhases = {kNrmCentroids, 3}, kClPhases = {kClDensity, kClusterPhases},
                     kPlanePhases = {kPlCompact, 6}, kRegPhases = {kRgNormals, 4}, kRegFramesPhases = {kRfNormals, 4},
                     kInsertPhases = {kInsValidate, 4}, kRemovePhases = {kRmValidate, 4}, kRaysPhases = {kRyClear, 2},
                     kKeptPhases = {kKnMark, 4};
constexpr int kRgSolve = 4;   // its public index
constexpr int kVoxMeta = 4;   // the words of VoxTable::meta
static_assert(kRegPhases.first + kRegPhases.count == kRfNormals && kRegFramesPhases.first + kRegFramesPhases.count == kInsValidate &&
              kInsertPhases.first + kInsertPhases.count == kRmValidate && kRemovePhases.first + kRemovePhases.count == kRyClear &&
              kRaysPhases.first + kRaysPhases.count == kKnMark && kKeptPhases.first + kKeptPhases.count == kAllPhases &&
              kClPhases.first + kClPhases.count == kPlCompact, "the ranges");

struct VoxState : mcimpl::CtxExt {
  // table (a power of two of slots), per-point arrays (points / chunks), per-voxel records
  DevBuf<unsigned long long> keys;
  DevBuf<uint32_t> first, vid;
  DevBuf<uint32_t> slot, vslot;
  DevBuf<uint8_t> flags;
  DevBuf<uint32_t> chunk;
  DevBuf<long long> sums;
  DevBuf<uint32_t> cnt;
  DevBuf<uint32_t> meta;
  // the last build
  bool built = false;
  int64_t M = 0;
  int64_t N = 0;        // the points the cloud holds: the build's, plus every insert's and merge's
  double h = 0.0, o[3] = {0, 0, 0};
  int log2cap = 0;      // the table's slots (0: the build was of an empty source and left no table)
  int shift = 0;
  uint32_t mask = 0;
  int64_t growths = 0;  // the times an insert or a merge made a new table since the build
  EventPairs ev[kAllPhases];   // by phase, of every stage
  // the normals of the last build: its centroids by voxel (written by the first mc_voxel_normals after the
  // build), the voxels the cap applies to and their number
  DevBuf<double> cent;
  bool cent_current = false;
  DevBuf<uint32_t> capped;
  DevBuf<uint32_t> n_capped;
  // the last clustering of the last build: the union-find word and the label of every voxel (the cluster's
  // number, kClusterNone for noise), the roots per workgroup, and K
  DevBuf<uint32_t> cl_parent, cl_label, cl_chunk, cl_meta;
  bool cl_current = false;
  int64_t cl_K = 0;
  // the plane segmentation and the selection: the ascending voxel ids of a mask and their scan, the hypothesis
  // table, the scores, the inlier byte of every voxel under the last model, and the levels of the refit's tree
  DevBuf<uint32_t> pl_ids, pl_chunk, pl_meta, pl_score, pl_count;
  DevBuf<double> pl_hyp, pl_tree;
  DevBuf<int32_t> pl_samples;
  DevBuf<uint8_t> pl_mask;
  // the registration of a source against the cloud: the nearest voxel of every source point, the normals and
  // their neighbour counts by voxel id, and the levels of the 28-wide tree with the pair counter behind the last;
  // the solve is the host's, timed by its clock
  DevBuf<int32_t> rg_ids, rg_counts;
  DevBuf<double> rg_normals, rg_tree;
  double rg_solve_ms = 0.0;
  int64_t rg_solve_n = 0;
  // the frames of a batch registered together: a record per frame, the block maps of the first level and of the two
  // further ones, every frame's levels back to back, the history of every frame, and the frames still live
  DevBuf<RegFrame> rf_frames;
  DevBuf<int64_t> rf_map;
  DevBuf<double> rf_tree, rf_history;
  DevBuf<uint32_t> rf_live;
  // a removal: the keep byte of every voxel, the survivors' packed keys on their way into the cleared table, and
  // the word that takes their points
  DevBuf<uint8_t> rm_keep;
  DevBuf<unsigned long long> rm_keys, rm_points;
  // the rays of a call: the sensor positions of a batch's frames, and the skipped rays and the transitions walked
  DevBuf<double> ry_origins;
  DevBuf<unsigned long long> ry_meta;
  // the normals the cloud keeps across its edits (mc_voxel_keep_normals): their own rows and counts by voxel id (rg_normals
  // and rg_counts stay the scratch of a registration with other parameters), the two stamps of every voxel and the epoch of
  // the last edit (normals_core.hpp "kept normals"), the dirty list with its counter, and what the edits have recomputed.
  // 48 B per voxel: 36 of rows, 8 of stamps, 4 of list.  While kn_on, every edit leaves cent current
  DevBuf<double> kn_normals;
  DevBuf<int32_t> kn_counts;
  DevBuf<uint32_t> kn_touched, kn_dirty, kn_list, kn_meta;
  bool kn_on = false;
  double kn_radius = 0.0;
  int32_t kn_max_nn = 0;
  uint32_t kn_epoch = 0;
  int64_t kn_full = 0, kn_last = 0, kn_total = 0;   // since the build: full passes, rows of the last edit, rows of all edits

  // with the context (mc_voxel_release has recycled the pairs into the context's pool before)
  ~VoxState() override {
    for (auto& v : ev) ev_destroy(v);
  }
};

// the context's state (made on demand)
VoxState* state_of(mc_ctx* c, bool create) { return ctx_ext<VoxState>(c, mcimpl::kSlotVoxel, create); }

// the state of the live build, for the entry point `who`
int live_build(mc_ctx* c, const char* who, VoxState** s) {
  *s = state_of(c, false);
  if (!*s || !(*s)->built) return fail(MC_ERR_STATE, "%s needs a successful mc_voxel_build_* first", who);
  return MC_OK;
}

// a stage's mc_timing_read_*
int read_phases(mc_ctx* c, PhaseRange p, double* ms_phase, int64_t* launches) {
  VoxState* s = state_of(c, false);
  return read_timing_phases(c, s ? s->ev + p.first : nullptr, p.count, ms_phase, launches);
}

// ---- views of the state: what the kernels' argument structs take of it ------------------------------------------------
// the per-voxel sums and the grid, the outputs left null
VoxOut out_of(const VoxState* s) {
  VoxOut a = {};
  a.keys = s->keys; a.vslot = s->vslot; a.sums = s->sums; a.cnt = s->cnt;
  a.M = s->M;
  a.h = s->h;
  std::copy_n(s->o, 3, a.o);
  return a;
}

// the key table and the centroids (written by centroids())
NormalsGrid grid_of(const VoxState* s) {
  NormalsGrid g = {};
  g.keys = s->keys; g.vid = s->vid; g.cent = s->cent;
  g.shift = s->shift; g.mask = s->mask;
  return g;
}

// the cells a search of `radius` looks at on every axis, each way
int window_cells(const VoxState* s, double radius) { return std::max(1, (int)std::ceil(radius / s->h)); }

NormalsQuery query_of(const VoxState* s, double radius, int32_t max_nn) {
  NormalsQuery q = {};
  q.R = window_cells(s, radius);
  q.max_nn = max_nn;
  q.r2 = radius * radius;
  return q;
}

// a search radius (`name`: radius, eps, max_distance) against the widest window the kernels walk
int check_window(const VoxState* s, double v, const char* name) {
  CHECK_ARG(v / s->h <= (double)kNormalsMaxR,
            "%s %g is %g voxels of %g and the search window takes at most %d: voxelise coarser or shrink the radius", name, v,
            v / s->h, s->h, kNormalsMaxR);
  return MC_OK;
}

// ---- small things ------------------------------------------------------------------------------------------------------
uint32_t blocks_of(int64_t n) { return (uint32_t)((n + kVoxBlock - 1) / kVoxBlock); }

// these bytes back to the host, and wait: a call's synchronisation
int copy_back(mc_ctx* c, void* host, const void* dev, size_t bytes) {
  HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

// The scan of n per-workgroup counts, queued inside the caller's timed region between the kernels that count and
// those that rank: chunk -> its exclusive scan in place, meta[1] the total.  The caller brings meta back with its one
// synchronisation (copy_back) and bounds the total in its own words
void scan_counts(mc_ctx* c, uint32_t* chunk, int64_t n, uint32_t* meta) {
  hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(kVoxBlock), 0, c->stream, chunk, n, meta);
}

// RegPose <-> a row-major 4 x 4 (the last row is the caller's to check or to write)
void pose_from_rows(const double* m, RegPose* T) {
  for (int r = 0; r < 3; ++r) {
    std::copy_n(m + 4 * r, 3, T->R + 3 * r);
    T->t[r] = m[4 * r + 3];
  }
}
void pose_to_rows(const RegPose& T, double* m) {
  for (int r = 0; r < 3; ++r) {
    std::copy_n(T.R + 3 * r, 3, m + 4 * r);
    m[4 * r + 3] = T.t[r];
  }
  m[12] = m[13] = m[14] = 0.0;
  m[15] = 1.0;
}

int check_grid(double voxel, const double* origin) {
  CHECK_ARG(std::isfinite(voxel) && voxel > 0.0, "voxel must be finite and > 0 (got %g)", voxel);
  CHECK_ARG(origin, "origin is NULL");
  for (int k = 0; k < 3; ++k) CHECK_ARG(std::isfinite(origin[k]), "origin must be finite (axis %d: %g)", k, origin[k]);
  return MC_OK;
}

// ---- the normals a cloud keeps across its edits (defined behind normals_run) --------------------------------------------
// An edit of a cloud with kept normals (s->kn_on), in this order: kept_reserve when it adds voxels, kept_begin_edit,
// its mark (kept_mark_items once the records are in; a removal marks and carries in keep_voxels), and kept_refresh
// once s->M and the table are the edited cloud's and every centroid is current.
int kept_reserve(mc_ctx* c, VoxState* s, int64_t keep, int64_t M);
int kept_begin_edit(mc_ctx* c, VoxState* s, int64_t M);
int kept_mark_items(mc_ctx* c, VoxState* s, int64_t M, int64_t n);
int kept_refresh(mc_ctx* c, VoxState* s);

// no normals kept any more, their blocks given back (the stream has drained, or nothing queued reads them)
void kept_free(VoxState* s) {
  s->kn_on = false;
  s->kn_normals.reset();
  s->kn_counts.reset();
  s->kn_touched.reset();
  s->kn_dirty.reset();
  s->kn_list.reset();
  s->kn_meta.reset();
}

// the build over n points of src; *bad: the lowest refused point (-1: none)
template <bool BATCH>
int build(mc_ctx* c, VoxSrc src, int64_t n, int64_t lanes, int64_t* n_voxels, int64_t* bad) {
  *bad = -1;
  *n_voxels = 0;
  VoxState* s = state_of(c, true);
  s->built = false;
  s->cent_current = false;
  s->cl_current = false;
  if (s->kn_normals) {   // a new build keeps no normals, and does not carry their 48 B per voxel along
    HIPCHK(hipStreamSynchronize(c->stream));
    kept_free(s);
  }
  s->kn_on = false;
  s->kn_full = s->kn_last = s->kn_total = 0;
  s->M = 0;
  s->N = 0;
  s->log2cap = 0;
  s->growths = 0;
  s->h = src.h;
  std::copy_n(src.o, 3, s->o);
  if (n == 0) { s->built = true; return MC_OK; }
  int log2cap = 6;
  while (((int64_t)1 << log2cap) < 2 * n) ++log2cap;   // n < 2^31: at most 2^32 slots
  const size_t cap = (size_t)1 << log2cap;
  const int64_t n_chunks = (n + kVoxChunk - 1) / kVoxChunk;
  if (!s->meta) if (int r = s->meta.alloc(kVoxMeta)) return r;
  if (int r = ctx_reserve(c, s->keys, cap)) return r;
  if (int r = ctx_reserve(c, s->first, cap)) return r;
  if (int r = ctx_reserve(c, s->vid, cap)) return r;
  if (int r = ctx_reserve(c, s->slot, (size_t)n)) return r;
  if (int r = ctx_reserve(c, s->vslot, (size_t)n)) return r;
  if (int r = ctx_reserve(c, s->flags, (size_t)n_chunks * kVoxBlock)) return r;
  if (int r = ctx_reserve(c, s->chunk, (size_t)n_chunks)) return r;
  VoxTable t;
  t.keys = s->keys; t.first = s->first; t.vid = s->vid; t.slot = s->slot;
  t.shift = 64 - log2cap;
  t.mask = (uint32_t)(cap - 1);
  t.meta = s->meta;
  s->shift = t.shift;
  s->mask = t.mask;
  const dim3 blk(kVoxBlock), pgrid(blocks_of(lanes)), cgrid((uint32_t)n_chunks);
  {
    TimedRegion tr(c, &s->ev[kInsert], c->stream);
    HIPCHK(hipMemsetAsync(s->keys, 0xFF, cap * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(s->first, 0xFF, cap * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->meta, 0xFF, 2 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_vox_insert<BATCH>, pgrid, blk, 0, c->stream, src, t);
  }
  {
    TimedRegion tr(c, &s->ev[kRank], c->stream);
    hipLaunchKernelGGL(k_vox_flag<false>, cgrid, blk, 0, c->stream, t, n, s->flags, s->chunk);
    scan_counts(c, s->chunk, n_chunks, s->meta);
    hipLaunchKernelGGL(k_vox_rank<false>, cgrid, blk, 0, c->stream, t, n, (const uint8_t*)s->flags, (const uint32_t*)s->chunk,
                       s->vslot, 0u);
  }
  HIPCHK(hipGetLastError());
  uint32_t meta[2] = {0, 0};
  if (int r = copy_back(c, meta, s->meta, sizeof meta)) return r;
  if (meta[0] != kVoxNone) {
    *bad = (int64_t)meta[0];
    return MC_ERR_INVALID;   // the caller words the message (frame / index or row)
  }
  const int64_t M = (int64_t)meta[1];
  if (M < 1 || M > n) return fail(MC_ERR_STATE, "voxel build: %lld voxels of %lld points", (long long)M, (long long)n);
  if (int r = ctx_reserve(c, s->sums, kVoxRec * (size_t)M)) return r;
  if (int r = ctx_reserve(c, s->cnt, (size_t)M)) return r;
  {
    TimedRegion tr(c, &s->ev[kAccumulate], c->stream);
    HIPCHK(hipMemsetAsync(s->sums, 0, kVoxRec * (size_t)M * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(s->cnt, 0, (size_t)M * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_vox_accumulate<BATCH>, pgrid, blk, 0, c->stream, src, t, s->sums, s->cnt);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  s->M = M;
  s->N = n;
  s->log2cap = log2cap;
  s->built = true;
  *n_voxels = M;
  return MC_OK;
}

// ---- growing the live cloud -------------------------------------------------------------------------------------------
// the view of the state's table the kernels take
VoxTable table_of(const VoxState* s) {
  VoxTable t;
  t.keys = s->keys; t.first = s->first; t.vid = s->vid; t.slot = s->slot;
  t.shift = s->shift;
  t.mask = s->mask;
  t.meta = s->meta;
  return t;
}

// A fresh table of 2^log2cap slots holding the cloud's M voxels (the invariant of voxel.hpp's header): the keys
// re-inserted by voxel through vslot, queued; the stream drains before the old blocks go back
int grow_table(mc_ctx* c, VoxState* s, int log2cap) {
  const size_t cap = (size_t)1 << log2cap;
  DevBuf<unsigned long long> keys;
  DevBuf<uint32_t> first, vid;
  if (int r = keys.alloc(cap)) return r;
  if (int r = first.alloc(cap)) return r;
  if (int r = vid.alloc(cap)) return r;
  VoxTable t = {};
  t.keys = keys; t.first = first; t.vid = vid;
  t.shift = 64 - log2cap;
  t.mask = (uint32_t)(cap - 1);
  HIPCHK(hipMemsetAsync(keys, 0xFF, cap * sizeof(unsigned long long), c->stream));
  HIPCHK(hipMemsetAsync(first, 0xFF, cap * sizeof(uint32_t), c->stream));
  if (s->M > 0)
    hipLaunchKernelGGL(k_vox_rehash, dim3(blocks_of(s->M)), dim3(kVoxBlock), 0, c->stream, (const unsigned long long*)s->keys.get(),
                       s->vslot.get(), s->M, t);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  s->keys = std::move(keys);
  s->first = std::move(first);
  s->vid = std::move(vid);
  s->log2cap = log2cap;
  s->shift = t.shift;
  s->mask = t.mask;
  ++s->growths;
  return MC_OK;
}

// The n items of src into the live cloud s (include/mcdeskew.h "growing a voxel cloud").  points: what they hold when
// the host knows it (a point each), -1 for records, whose counts the validation adds up.  *bad: the lowest refused
// item (-1: none; the caller words the message); a refused call has not touched the table
template <int KIND, typename Src>
int insert(mc_ctx* c, VoxState* s, Src src, int64_t n, int64_t lanes, int64_t points, int64_t* n_new, int64_t* bad) {
  *bad = -1;
  *n_new = 0;
  s->kn_last = 0;   // a refused call and one without items recompute no kept row
  if (n == 0) return MC_OK;
  if constexpr (KIND != kVoxRecords) {   // points are quantised on the cloud's own grid
    src.h = s->h;
    std::copy_n(s->o, 3, src.o);
  }
  if (!s->meta) if (int r = s->meta.alloc(kVoxMeta)) return r;
  const int64_t n_chunks = (n + kVoxChunk - 1) / kVoxChunk;
  const dim3 blk(kVoxBlock), pgrid(blocks_of(lanes)), cgrid((uint32_t)n_chunks);
  uint32_t meta[kVoxMeta] = {0, 0, 0, 0};
  {
    TimedRegion tr(c, &s->ev[kInsValidate], c->stream);
    HIPCHK(hipMemsetAsync(s->meta, 0xFF, 2 * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->meta + 2, 0, 2 * sizeof(uint32_t), c->stream));
    // records are validated a chunk per workgroup (k_vox_validate), points a group per lane
    hipLaunchKernelGGL((k_vox_validate<KIND, Src>), KIND == kVoxRecords ? cgrid : pgrid, blk, 0, c->stream, src, s->meta.get());
  }
  HIPCHK(hipGetLastError());
  if (int r = copy_back(c, meta, s->meta, sizeof meta)) return r;
  if (meta[0] != kVoxNone) {
    *bad = (int64_t)meta[0];
    return MC_ERR_INVALID;
  }
  if (points < 0) points = (int64_t)((uint64_t)meta[2] | (uint64_t)meta[3] << 32);
  if (points < n || s->N + points >= kVoxelPointsEnd)
    return fail(MC_ERR_INVALID, "the cloud holds %lld points and the call brings %lld: a cloud takes fewer than 2^31 in all",
                (long long)s->N, (long long)points);
  const int64_t M = s->M;
  const int log2cap = voxel_table_log2(M, n, s->log2cap);
  if (int r = ctx_reserve(c, s->slot, (size_t)n)) return r;
  if (int r = ctx_reserve(c, s->flags, (size_t)n_chunks * kVoxBlock)) return r;
  if (int r = ctx_reserve(c, s->chunk, (size_t)n_chunks)) return r;
  VoxTable t;
  {
    TimedRegion tr(c, &s->ev[kInsInsert], c->stream);
    if (log2cap != s->log2cap) if (int r = grow_table(c, s, log2cap)) return r;   // the same cloud in a larger table
    s->built = false;   // from here the call's keys go in: a failure that is no refusal (memory, HIP) leaves no live build
    t = table_of(s);
    hipLaunchKernelGGL((k_vox_insert_live<KIND, Src>), pgrid, blk, 0, c->stream, src, t);
  }
  {
    TimedRegion tr(c, &s->ev[kInsRank], c->stream);
    hipLaunchKernelGGL(k_vox_flag<true>, cgrid, blk, 0, c->stream, t, n, s->flags, s->chunk);
    scan_counts(c, s->chunk, n_chunks, s->meta);
  }
  HIPCHK(hipGetLastError());
  // the call's second synchronisation: the new voxels, which size the records
  if (int r = copy_back(c, meta, s->meta, 2 * sizeof(uint32_t))) return r;
  const int64_t fresh = (int64_t)meta[1], Mn = M + fresh;
  if (fresh > n || Mn >= kVoxelPointsEnd) return fail(MC_ERR_STATE, "voxel insert: %lld new voxels of %lld items", (long long)fresh, (long long)n);
  if (int r = ctx_reserve_keep(c, s->vslot, (size_t)M, (size_t)Mn)) return r;
  if (int r = ctx_reserve_keep(c, s->sums, kVoxRec * (size_t)M, kVoxRec * (size_t)Mn)) return r;
  if (int r = ctx_reserve_keep(c, s->cnt, (size_t)M, (size_t)Mn)) return r;
  {
    TimedRegion tr(c, &s->ev[kInsRank], c->stream);
    hipLaunchKernelGGL(k_vox_rank<true>, cgrid, blk, 0, c->stream, t, n, (const uint8_t*)s->flags, (const uint32_t*)s->chunk,
                       s->vslot, (uint32_t)M);
  }
  {
    TimedRegion tr(c, &s->ev[kInsAccumulate], c->stream);
    if (fresh > 0) {
      HIPCHK(hipMemsetAsync(s->sums + kVoxRec * M, 0, kVoxRec * (size_t)fresh * sizeof(long long), c->stream));
      HIPCHK(hipMemsetAsync(s->cnt + M, 0, (size_t)fresh * sizeof(uint32_t), c->stream));
    }
    hipLaunchKernelGGL((k_vox_accumulate_items<KIND, Src>), pgrid, blk, 0, c->stream, src, t, s->sums.get(), s->cnt.get());
  }
  HIPCHK(hipGetLastError());
  if (s->kn_on) {   // the records are in: the touched voxels' centroids and the dirty set (its refresh below)
    if (int r = kept_reserve(c, s, M, Mn)) return r;
    if (int r = kept_begin_edit(c, s, Mn)) return r;
    if (int r = kept_mark_items(c, s, Mn, n)) return r;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  s->M = Mn;
  s->N += points;
  s->built = true;
  s->cent_current = s->kn_on;   // as a new build: the next analysis sees the grown cloud (kept normals: the mark has)
  s->cl_current = false;
  *n_new = fresh;
  return s->kn_on ? kept_refresh(c, s) : MC_OK;
}

// the frame of dense point p of a batch: the last one starting at or before it (empty frames start where the next
// begins and come earlier in the order)
int32_t frame_of(const mc_batch* in, int64_t p) {
  return (int32_t)(std::upper_bound(in->doff.begin(), in->doff.begin() + in->F + 1, p) - in->doff.begin()) - 1;
}

VoxSrc batch_source(const mc_batch* in) {
  VoxSrc src = {};
  src.cols = in->d_cols; src.C = in->C; src.F = in->F;
  src.poff = in->d_poff; src.doff = in->d_doff; src.counts = in->d_counts;
  src.P = in->P;
  src.n = in->N;
  return src;
}

const char* kRefused =
    "a coordinate or (v - origin) / voxel is not finite, a voxel index is outside [-2^20, 2^20), or the intensity is "
    "not finite or beyond +-65536";

// a: out_of(s) with its outputs set
int emit(mc_ctx* c, VoxState* s, const VoxOut& a, bool batch, int64_t P) {
  const int64_t lanes = batch ? P / 4 : s->M;
  if (lanes == 0) return MC_OK;
  const dim3 blk(kVoxBlock), grid(blocks_of(lanes));
  {
    TimedRegion tr(c, &s->ev[kFinalise], c->stream);
    if (batch) hipLaunchKernelGGL(k_vox_emit_batch, grid, blk, 0, c->stream, a, P);
    else hipLaunchKernelGGL(k_vox_emit_rows, grid, blk, 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return MC_OK;
}

// the centroids by voxel id of the live build (M > 0), written once per build: what the window walks of the
// normals and of the clustering read
int centroids(mc_ctx* c, VoxState* s) {
  const int64_t M = s->M;
  if (int r = ctx_reserve(c, s->cent, kNormalsCent * (size_t)M)) return r;
  if (s->cent_current) return MC_OK;
  {
    TimedRegion tr(c, &s->ev[kNrmCentroids], c->stream);
    hipLaunchKernelGGL(k_nrm_centroids, dim3(blocks_of(M)), dim3(kVoxBlock), 0, c->stream, out_of(s), s->cent.get());
  }
  HIPCHK(hipGetLastError());
  s->cent_current = true;
  return MC_OK;
}

// the ascending voxel ids of the set bytes of d_mask (M > 0) into pl_ids, and their number (one synchronisation)
int compact(mc_ctx* c, VoxState* s, const uint8_t* d_mask, int phase, int64_t* n) {
  const int64_t M = s->M;
  const uint32_t blocks = blocks_of(M);
  if (int r = ctx_reserve(c, s->pl_ids, (size_t)M)) return r;
  if (int r = ctx_reserve(c, s->pl_chunk, (size_t)blocks)) return r;
  if (!s->pl_meta) if (int r = s->pl_meta.alloc(2)) return r;
  {
    TimedRegion tr(c, &s->ev[phase], c->stream);
    hipLaunchKernelGGL(k_pl_flag, dim3(blocks), dim3(kVoxBlock), 0, c->stream, d_mask, M, s->pl_chunk.get());
    scan_counts(c, s->pl_chunk, blocks, s->pl_meta);
    hipLaunchKernelGGL(k_pl_scatter, dim3(blocks), dim3(kVoxBlock), 0, c->stream, d_mask, M, (const uint32_t*)s->pl_chunk.get(),
                       s->pl_ids.get());
  }
  HIPCHK(hipGetLastError());
  uint32_t meta[2] = {0, 0};
  if (int r = copy_back(c, meta, s->pl_meta, sizeof meta)) return r;
  if ((int64_t)meta[1] > M) return fail(MC_ERR_STATE, "voxel mask: %u set bytes of %lld voxels", meta[1], (long long)M);
  *n = (int64_t)meta[1];
  return MC_OK;
}

// ---- shrinking the live cloud -----------------------------------------------------------------------------------------
// The voxels of the live cloud (M > 0) whose byte in rm_keep is set stay, in their order, as voxels 0 .. M' - 1
// (voxel.hpp "taking voxels and points out"): the survivors' ids, their records and keys compacted into fresh arrays,
// the table cleared (shrunk by voxel_table_shrink_log2's rule) and refilled.  M' == M: nothing is touched.  Two
// synchronisations: M', and the survivors' points with the end of the refill, before the old blocks go back.
// Kept normals: the windows of the removed cells are stamped on the old ids before the refill (marked: a subtraction's
// items have done it), the kept rows go to the survivors' new ids with the records, every centroid is written again (a
// removal is a pass over the cloud anyway) and the stamped survivors are refreshed.
int keep_voxels(mc_ctx* c, VoxState* s, int64_t* n_removed, bool marked = false) {
  *n_removed = 0;
  const int64_t M = s->M;
  int64_t Mk = 0;
  if (int r = compact(c, s, s->rm_keep, kRmCompact, &Mk)) return r;
  if (Mk == M) return MC_OK;
  const int log2cap = voxel_table_shrink_log2(Mk, s->log2cap);
  const size_t cap = (size_t)1 << log2cap;
  DevBuf<long long> sums;
  DevBuf<uint32_t> cnt;
  if (int r = sums.alloc(kVoxRec * (size_t)Mk)) return r;
  if (int r = cnt.alloc((size_t)Mk)) return r;
  if (int r = ctx_reserve(c, s->rm_keys, (size_t)Mk)) return r;
  if (!s->rm_points) if (int r = s->rm_points.alloc(1)) return r;
  DevBuf<unsigned long long> keys;   // of a shrink alone: a table of the same size is refilled in place
  DevBuf<uint32_t> first, vid;
  VoxTable t = table_of(s);
  if (log2cap != s->log2cap) {
    if (int r = keys.alloc(cap)) return r;
    if (int r = first.alloc(cap)) return r;
    if (int r = vid.alloc(cap)) return r;
    t.keys = keys; t.first = first; t.vid = vid;
    t.shift = 64 - log2cap;
    t.mask = (uint32_t)(cap - 1);
  }
  DevBuf<double> kn_normals;
  DevBuf<int32_t> kn_counts;
  DevBuf<uint32_t> kn_touched, kn_dirty;
  if (s->kn_on) {
    if (int r = kn_normals.alloc(4 * (size_t)Mk)) return r;
    if (int r = kn_counts.alloc((size_t)Mk)) return r;
    if (int r = kn_touched.alloc((size_t)Mk)) return r;
    if (int r = kn_dirty.alloc((size_t)Mk)) return r;
    if (!marked) if (int r = kept_begin_edit(c, s, M)) return r;
  }
  s->built = false;   // from here the records and the table change: a failure leaves no live build
  if (s->kn_on) {
    if (!marked) {
      NrmMarkArgs m = {};
      m.g = grid_of(s);
      m.rec = out_of(s);
      m.keep = s->rm_keep; m.n = M;
      m.R = window_cells(s, s->kn_radius);
      m.epoch = s->kn_epoch;
      m.dirty = s->kn_dirty;
      TimedRegion tr(c, &s->ev[kKnMark], c->stream);
      hipLaunchKernelGGL(k_nrm_mark<true>, dim3(blocks_of(M)), dim3(kVoxBlock), 0, c->stream, m);
    }
    NrmCarryArgs a = {};
    a.ids = s->pl_ids; a.M_keep = Mk;
    a.normals = s->kn_normals; a.counts = s->kn_counts; a.dirty = s->kn_dirty;
    a.epoch = s->kn_epoch;
    a.normals_out = kn_normals; a.counts_out = kn_counts;
    a.list = s->kn_list; a.n_list = s->kn_meta;
    TimedRegion tr(c, &s->ev[kKnCarry], c->stream);
    HIPCHK(hipMemsetAsync(s->kn_meta, 0, sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(kn_touched, 0, (size_t)std::max<int64_t>(Mk, 1) * sizeof(uint32_t), c->stream));   // no stamp is an epoch to come
    HIPCHK(hipMemsetAsync(kn_dirty, 0, (size_t)std::max<int64_t>(Mk, 1) * sizeof(uint32_t), c->stream));
    if (Mk > 0) hipLaunchKernelGGL(k_nrm_carry, dim3(blocks_of(Mk)), dim3(kVoxBlock), 0, c->stream, a);
  }
  {
    TimedRegion tr(c, &s->ev[kRmCompact], c->stream);
    HIPCHK(hipMemsetAsync(s->rm_points, 0, sizeof(unsigned long long), c->stream));
    VoxCompact a = {};
    a.ids = s->pl_ids; a.M_keep = Mk;
    a.keys = s->keys; a.vslot = s->vslot; a.sums = s->sums; a.cnt = s->cnt;
    a.sums_out = sums; a.cnt_out = cnt; a.keys_out = s->rm_keys; a.points = s->rm_points;
    if (Mk > 0) hipLaunchKernelGGL(k_vox_compact, dim3(blocks_of(Mk)), dim3(kVoxBlock), 0, c->stream, a);
    HIPCHK(hipMemsetAsync(t.keys, 0xFF, cap * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(t.first, 0xFF, cap * sizeof(uint32_t), c->stream));
    if (Mk > 0)
      hipLaunchKernelGGL(k_vox_refill, dim3(blocks_of(Mk)), dim3(kVoxBlock), 0, c->stream, (const unsigned long long*)s->rm_keys.get(),
                         s->vslot.get(), Mk, t);
  }
  HIPCHK(hipGetLastError());
  unsigned long long points = 0;
  if (int r = copy_back(c, &points, s->rm_points, sizeof points)) return r;   // the stream has drained
  if (points > (unsigned long long)s->N || (int64_t)points < Mk)
    return fail(MC_ERR_STATE, "voxel remove: %llu points in %lld voxels kept of a cloud of %lld points", points, (long long)Mk,
                (long long)s->N);
  s->sums = std::move(sums);
  s->cnt = std::move(cnt);
  if (log2cap != s->log2cap) {   // a shrink is no growth: growths stays
    s->keys = std::move(keys);
    s->first = std::move(first);
    s->vid = std::move(vid);
    s->log2cap = log2cap;
    s->shift = t.shift;
    s->mask = t.mask;
  }
  s->M = Mk;
  s->N = (int64_t)points;
  s->cent_current = false;   // as an insert: the next analysis sees the shrunk cloud
  s->cl_current = false;
  s->built = true;
  *n_removed = M - Mk;
  if (!s->kn_on) return MC_OK;
  s->kn_normals = std::move(kn_normals);
  s->kn_counts = std::move(kn_counts);
  s->kn_touched = std::move(kn_touched);
  s->kn_dirty = std::move(kn_dirty);
  if (Mk == 0) {   // nothing is left to refresh; the cloud of no voxels keeps no rows
    s->cent_current = true;
    return MC_OK;
  }
  if (int r = centroids(c, s)) { s->kn_on = false; return r; }
  return kept_refresh(c, s);
}

// the keep bytes of the live cloud (M > 0), queued: d_mask's clear bytes, or (null) the voxels that hold points
int keep_flags(mc_ctx* c, VoxState* s, const uint8_t* d_mask) {
  if (int r = ctx_reserve(c, s->rm_keep, (size_t)s->M)) return r;
  {
    TimedRegion tr(c, &s->ev[kRmCompact], c->stream);
    if (d_mask)
      hipLaunchKernelGGL(k_vox_keep<true>, dim3(blocks_of(s->M)), dim3(kVoxBlock), 0, c->stream, d_mask, (const uint32_t*)nullptr, s->M,
                         s->rm_keep.get());
    else
      hipLaunchKernelGGL(k_vox_keep<false>, dim3(blocks_of(s->M)), dim3(kVoxBlock), 0, c->stream, (const uint8_t*)nullptr,
                         (const uint32_t*)s->cnt.get(), s->M, s->rm_keep.get());
  }
  HIPCHK(hipGetLastError());
  return MC_OK;
}

// why a subtraction refused (include/mcdeskew.h MC_VOXEL_SUB_*)
struct SubRefusal {
  int64_t item = -1;     // the lowest refused item (-1: none, as for the points)
  int32_t why = MC_VOXEL_SUB_OK;
  int32_t key[3] = {0, 0, 0};   // MC_VOXEL_SUB_REMAINDER: the voxel
};

// The n items of src out of the live cloud s (include/mcdeskew.h "shrinking a voxel cloud").  points: as insert's.
// *ref: what was refused; a refused call leaves every record as it was
template <int KIND, typename Src>
int subtract(mc_ctx* c, VoxState* s, Src src, int64_t n, int64_t lanes, int64_t points, int64_t* n_emptied, SubRefusal* ref) {
  *ref = SubRefusal();
  *n_emptied = 0;
  s->kn_last = 0;   // as an insert's
  if (n == 0) return MC_OK;
  if constexpr (KIND != kVoxRecords) {   // points are quantised on the cloud's own grid
    src.h = s->h;
    std::copy_n(s->o, 3, src.o);
  }
  if (!s->meta) if (int r = s->meta.alloc(kVoxMeta)) return r;
  if (int r = ctx_reserve(c, s->slot, (size_t)n)) return r;
  const int64_t n_chunks = (n + kVoxChunk - 1) / kVoxChunk;
  const dim3 blk(kVoxBlock), pgrid(blocks_of(lanes)), cgrid((uint32_t)n_chunks), igrid(blocks_of(n));
  VoxTable t = table_of(s);
  if (s->log2cap == 0) t.keys = nullptr;   // the cloud of an empty source has no table: it holds no item's voxel
  uint32_t meta[kVoxMeta] = {0, 0, 0, 0};
  {
    TimedRegion tr(c, &s->ev[kRmValidate], c->stream);
    HIPCHK(hipMemsetAsync(s->meta, 0xFF, 2 * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->meta + 2, 0, 2 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL((k_vox_sub_validate<KIND, Src>), KIND == kVoxRecords ? cgrid : pgrid, blk, 0, c->stream, src, t, s->meta.get());
  }
  HIPCHK(hipGetLastError());
  if (int r = copy_back(c, meta, s->meta, sizeof meta)) return r;
  if (meta[0] != kVoxNone || meta[1] != kVoxNone) {   // an item is one or the other: the words differ
    ref->item = (int64_t)std::min(meta[0], meta[1]);
    ref->why = meta[0] < meta[1] ? MC_VOXEL_SUB_ITEM : MC_VOXEL_SUB_MISSING;
    return MC_ERR_INVALID;
  }
  if (points < 0) points = (int64_t)((uint64_t)meta[2] | (uint64_t)meta[3] << 32);
  if (points > s->N) {
    ref->why = MC_VOXEL_SUB_POINTS;
    return fail(MC_ERR_INVALID, "the call brings %lld points and the cloud holds %lld: more points than it holds cannot leave (the "
                "cloud is unchanged)", (long long)points, (long long)s->N);
  }
  s->built = false;   // from here the records change: a failure that is no refusal leaves no live build
  {
    TimedRegion tr(c, &s->ev[kRmApply], c->stream);
    hipLaunchKernelGGL((k_vox_sub_apply<KIND, Src>), pgrid, blk, 0, c->stream, src, t, s->sums.get(), s->cnt.get(), -1);
  }
  {
    TimedRegion tr(c, &s->ev[kRmCheck], c->stream);
    HIPCHK(hipMemsetAsync(s->meta, 0xFF, sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->meta + 1, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_vox_sub_check, igrid, blk, 0, c->stream, t, n, (const long long*)s->sums.get(), (const uint32_t*)s->cnt.get(),
                       s->meta.get());
  }
  HIPCHK(hipGetLastError());
  // the call's second synchronisation: whether every record is still a set of points, and whether one is empty
  if (int r = copy_back(c, meta, s->meta, 2 * sizeof(uint32_t))) return r;
  if (meta[0] != kVoxNone) {   // the items come back: integers, so every record is what it was
    if ((int64_t)meta[0] >= n) return fail(MC_ERR_STATE, "voxel subtract: item %u of %lld", meta[0], (long long)n);
    {
      TimedRegion tr(c, &s->ev[kRmApply], c->stream);
      hipLaunchKernelGGL((k_vox_sub_apply<KIND, Src>), pgrid, blk, 0, c->stream, src, t, s->sums.get(), s->cnt.get(), 1);
    }
    HIPCHK(hipGetLastError());
    uint32_t at = 0;
    unsigned long long key = 0;
    if (int r = copy_back(c, &at, s->slot + meta[0], sizeof at)) return r;
    if (at > s->mask) return fail(MC_ERR_STATE, "voxel subtract: slot %u of a table of %u", at, s->mask);
    if (int r = copy_back(c, &key, s->keys + at, sizeof key)) return r;
    voxel_unpack(key, ref->key);
    ref->item = (int64_t)meta[0];
    ref->why = MC_VOXEL_SUB_REMAINDER;
    s->built = true;
    return MC_ERR_INVALID;
  }
  if (s->kn_on) {   // the records are what they will be: the touched voxels (the emptied ones too) mark their windows
    if (int r = kept_begin_edit(c, s, s->M)) return r;
    if (int r = kept_mark_items(c, s, s->M, n)) return r;
  }
  s->N -= points;
  s->cent_current = s->kn_on;   // as an insert: the next analysis sees the shrunk cloud
  s->cl_current = false;
  s->built = true;
  if (meta[1] == 0) return s->kn_on ? kept_refresh(c, s) : MC_OK;   // no voxel emptied: no pass over the cloud or the table
  const int64_t left = s->N;
  // a failure from here leaves the cloud live or not, but never with kept rows its marked items have not refreshed,
  // nor with the emptied voxels' centroids taken for current
  if (int r = keep_flags(c, s, nullptr)) { s->kn_on = false; s->cent_current = false; return r; }
  if (int r = keep_voxels(c, s, n_emptied, true)) { s->kn_on = false; s->cent_current = false; return r; }
  if (s->N != left) {
    s->built = false;
    return fail(MC_ERR_STATE, "voxel subtract: the voxels kept hold %lld points of %lld", (long long)s->N, (long long)left);
  }
  return MC_OK;
}

// the message of a refused item (`item`: how its source names it; rule: what the filter or the record check refuses)
int subtract_refused(const char* item, const SubRefusal& ref, const char* rule) {
  switch (ref.why) {
    case MC_VOXEL_SUB_ITEM:
      return fail(MC_ERR_INVALID, "%s (the lowest refused; the cloud is unchanged): %s", item, rule);
    case MC_VOXEL_SUB_MISSING:
      return fail(MC_ERR_INVALID, "%s (the lowest refused; the cloud is unchanged): the cloud holds no voxel of this item", item);
    default:
      return fail(MC_ERR_INVALID,
                  "%s (the lowest of its voxel; the cloud is unchanged): voxel (%d, %d, %d) would be left with a record that no set "
                  "of points sums to: a count below 0, a count of 0 with a sum left over, a coordinate sum outside 0 .. count * 2^32 "
                  "or an intensity sum beyond +-count * 2^32", item, ref.key[0], ref.key[1], ref.key[2]);
  }
}

// pl_mask = the candidates inside (n, d) and their number (one synchronisation)
int plane_mask(mc_ctx* c, VoxState* s, const uint8_t* d_among, const double model[4], double bound, bool refined,
               int64_t* n_inliers) {
  PlaneMaskArgs a = {};
  a.cent = s->cent; a.among = d_among; a.M = s->M;
  std::copy_n(model, 3, a.n);
  a.d = model[3];
  a.bound = bound;
  a.refined = refined ? 1 : 0;
  a.mask = s->pl_mask; a.count = s->pl_count;
  {
    TimedRegion tr(c, &s->ev[kPlMask], c->stream);
    HIPCHK(hipMemsetAsync(s->pl_count, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_pl_mask, dim3(blocks_of(s->M)), dim3(kVoxBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  uint32_t count = 0;
  if (int r = copy_back(c, &count, s->pl_count, sizeof count)) return r;
  *n_inliers = (int64_t)count;
  return MC_OK;
}

// A tree of `width` sums over L leaves (a power of two >= 256): its levels lie back to back, the first of L / 256
// partials per sum, each next of a 256th, down to the first of fewer than 256: -> the words of all of them
size_t tree_words(int width, int64_t L) {
  size_t words = 0;
  for (int64_t cnt = L / kVoxBlock;; cnt /= kVoxBlock) {
    words += (size_t)width * cnt;
    if (cnt < kVoxBlock) break;
  }
  return words;
}

// the levels after the first (*cnt partials per sum at cur), queued: -> the last level, *cnt its partials per sum
template <int kW>
double* tree_levels(mc_ctx* c, double* cur, int64_t* cnt) {
  while (*cnt >= kVoxBlock) {
    double* next = cur + kW * *cnt;
    hipLaunchKernelGGL(k_pl_tree<kW>, dim3((uint32_t)(*cnt / kVoxBlock)), dim3(kVoxBlock), 0, c->stream, (const double*)cur, *cnt, next);
    cur = next;
    *cnt /= kVoxBlock;
  }
  return cur;
}

// fewer than 256 partials per sum are left (top[k * cnt + i], on the host): the last levels of the same tree, in place
void tree_top(double* top, int64_t cnt, int width, double* sums) {
  for (int k = 0; k < width; ++k) sums[k] = plane_tree(top + (size_t)k * cnt, cnt, 1);
}

// the nine tree sums of pl_mask's voxels about p0 (one synchronisation)
int plane_moments(mc_ctx* c, VoxState* s, const double p0[3], double sums[kPlaneSums]) {
  const int64_t L = plane_leaves(s->M);
  if (int r = ctx_reserve(c, s->pl_tree, tree_words(kPlaneSums, L))) return r;
  int64_t cnt = L / kVoxBlock;
  double* cur = s->pl_tree;
  {
    TimedRegion tr(c, &s->ev[kPlMoments], c->stream);
    hipLaunchKernelGGL(k_pl_moments, dim3((uint32_t)cnt), dim3(kVoxBlock), 0, c->stream, (const double*)s->cent.get(),
                       (const uint8_t*)s->pl_mask.get(), s->M, p0[0], p0[1], p0[2], cur);
    cur = tree_levels<kPlaneSums>(c, cur, &cnt);
  }
  HIPCHK(hipGetLastError());
  std::vector<double> top((size_t)kPlaneSums * cnt);
  if (int r = copy_back(c, top.data(), cur, top.size() * sizeof(double))) return r;
  tree_top(top.data(), cnt, kPlaneSums, sums);
  return MC_OK;
}

// what mc_voxel_normals refuses of its plain arguments
int normals_checks(double radius, int32_t max_nn, const double* viewpoint) {
  CHECK_ARG(std::isfinite(radius) && radius > 0.0, "radius must be finite and > 0 (got %g)", radius);
  CHECK_ARG(max_nn == 0 || (max_nn >= kNormalsMinNN && max_nn <= kNormalsMaxNN),
            "max_nn must be 0 (no cap) or in %d..%d (got %d)", kNormalsMinNN, kNormalsMaxNN, max_nn);
  if (viewpoint)
    for (int k = 0; k < 3; ++k)
      CHECK_ARG(std::isfinite(viewpoint[k]), "viewpoint must be finite (axis %d: %g)", k, viewpoint[k]);
  return MC_OK;
}

// The normals of the live build (include/mcdeskew.h mc_voxel_normals) for `who`; for_register: the window and cap
// phases are timed as the registration's normals phase, not as the normals' own; as_phase >= 0: as that phase
int normals_run(mc_ctx* c, double radius, int32_t max_nn, const double* viewpoint, double* d_normals, int32_t* d_counts,
                double* d_cov, const char* who, bool for_register, int as_phase = -1) {
  if (int r = normals_checks(radius, max_nn, viewpoint)) return r;
  CHECK_ARG(((uintptr_t)d_normals & 15) == 0 && ((uintptr_t)d_cov & 15) == 0, "d_normals and d_cov must be 16-byte aligned");
  VoxState* s;
  if (int r = live_build(c, who, &s)) return r;
  if (int r = check_window(s, radius, "radius")) return r;
  const int64_t M = s->M;
  if (M == 0) return MC_OK;
  CHECK_ARG(d_normals, "d_normals is NULL");
  DeviceGuard g(c->device);
  if (int r = centroids(c, s)) return r;
  if (int r = ctx_reserve(c, s->capped, (size_t)M)) return r;
  if (!s->n_capped) if (int r = s->n_capped.alloc(1)) return r;
  EventPairs* window = &s->ev[as_phase >= 0 ? as_phase : for_register ? kRgNormals : kNrmWindow];
  EventPairs* cap = &s->ev[as_phase >= 0 ? as_phase : for_register ? kRgNormals : kNrmCap];
  NrmArgs a = {};
  a.g = grid_of(s);
  a.vslot = s->vslot;
  a.M = M;
  a.q = query_of(s, radius, max_nn);
  a.has_viewpoint = viewpoint ? 1 : 0;
  if (viewpoint) std::copy_n(viewpoint, 3, a.viewpoint);
  a.normals = d_normals; a.counts = d_counts; a.cov = d_cov;
  a.capped = s->capped; a.n_capped = s->n_capped;
  {
    TimedRegion tr(c, window, c->stream);
    HIPCHK(hipMemsetAsync(s->n_capped, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_nrm_window<false>, dim3(blocks_of(M)), dim3(kVoxBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  // the one synchronisation: how many voxels the cap applies to (none: no third launch)
  uint32_t n_capped = 0;
  if (int r = copy_back(c, &n_capped, s->n_capped, sizeof n_capped)) return r;
  if ((int64_t)n_capped > M) return fail(MC_ERR_STATE, "voxel normals: %u capped voxels of %lld", n_capped, (long long)M);
  if (n_capped) {
    {
      TimedRegion tr(c, cap, c->stream);
      hipLaunchKernelGGL(k_nrm_cap, dim3((n_capped + kNrmCapBlock - 1) / kNrmCapBlock), dim3(kNrmCapBlock), 0, c->stream, a);
    }
    HIPCHK(hipGetLastError());
  }
  return MC_OK;
}

// ---- the normals a cloud keeps across its edits -------------------------------------------------------------------------
// The kept buffers (and the centroids, which stay current while normals are kept) for M voxels, the first `keep`
// voxels' contents kept; the stamps of the others start at 0, which is no epoch
int kept_reserve(mc_ctx* c, VoxState* s, int64_t keep, int64_t M) {
  const size_t k = (size_t)keep, m = (size_t)std::max<int64_t>(M, 1);
  if (int r = ctx_reserve_keep(c, s->kn_normals, 4 * k, 4 * m)) return r;
  if (int r = ctx_reserve_keep(c, s->kn_counts, k, m)) return r;
  if (int r = ctx_reserve_keep(c, s->kn_touched, k, m)) return r;
  if (int r = ctx_reserve_keep(c, s->kn_dirty, k, m)) return r;
  if (int r = ctx_reserve_keep(c, s->cent, kNormalsCent * k, kNormalsCent * m)) return r;
  if (int r = ctx_reserve(c, s->kn_list, m)) return r;
  if (!s->kn_meta) if (int r = s->kn_meta.alloc(1)) return r;
  if (M > keep) {
    HIPCHK(hipMemsetAsync(s->kn_touched + keep, 0, (size_t)(M - keep) * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->kn_dirty + keep, 0, (size_t)(M - keep) * sizeof(uint32_t), c->stream));
  }
  return MC_OK;
}

// the epoch of the edit that begins, over the M voxels that carry stamps (queued)
int kept_begin_edit(mc_ctx* c, VoxState* s, int64_t M) {
  bool clear = false;
  s->kn_epoch = normals_next_epoch(s->kn_epoch, &clear);
  if (clear && M > 0) {
    HIPCHK(hipMemsetAsync(s->kn_touched, 0, (size_t)M * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->kn_dirty, 0, (size_t)M * sizeof(uint32_t), c->stream));
  }
  return MC_OK;
}

// The mark of an insert's or a subtraction's n items (slot[i] filled, the records final) in the cloud of M voxels,
// queued: the touched voxels' centroids and the dirty list
int kept_mark_items(mc_ctx* c, VoxState* s, int64_t M, int64_t n) {
  NrmMarkArgs m = {};
  m.g = grid_of(s);
  m.rec = out_of(s);
  m.rec.M = M;
  m.slot = s->slot; m.n = n;
  m.R = window_cells(s, s->kn_radius);
  m.epoch = s->kn_epoch;
  m.touched = s->kn_touched; m.dirty = s->kn_dirty;
  m.list = s->kn_list; m.n_list = s->kn_meta;
  m.cent = s->cent;
  {
    TimedRegion tr(c, &s->ev[kKnMark], c->stream);
    HIPCHK(hipMemsetAsync(s->kn_meta, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_nrm_mark<false>, dim3(blocks_of(n)), dim3(kVoxBlock), 0, c->stream, m);
  }
  HIPCHK(hipGetLastError());
  return MC_OK;
}

// The rows of the dirty list estimated again on the edited cloud (s->M, the table and every centroid are its own).  Two
// synchronisations: the dirty count, and with a cap the capped count.  A failure leaves no kept normals
int kept_refresh_run(mc_ctx* c, VoxState* s) {
  const int64_t M = s->M;
  uint32_t n_dirty = 0;
  if (int r = copy_back(c, &n_dirty, s->kn_meta, sizeof n_dirty)) return r;
  if ((int64_t)n_dirty > M) return fail(MC_ERR_STATE, "kept normals: %u dirty voxels of %lld", n_dirty, (long long)M);
  s->kn_last = (int64_t)n_dirty;
  s->kn_total += (int64_t)n_dirty;
  if (n_dirty == 0) return MC_OK;
  if (int r = ctx_reserve(c, s->capped, (size_t)n_dirty)) return r;
  if (!s->n_capped) if (int r = s->n_capped.alloc(1)) return r;
  NrmArgs a = {};
  a.g = grid_of(s);
  a.vslot = s->vslot;
  a.M = M;
  a.q = query_of(s, s->kn_radius, s->kn_max_nn);
  a.normals = s->kn_normals; a.counts = s->kn_counts;
  a.capped = s->capped; a.n_capped = s->n_capped;
  a.list = s->kn_list; a.n_list = (int64_t)n_dirty;
  {
    TimedRegion tr(c, &s->ev[kKnWindow], c->stream);
    HIPCHK(hipMemsetAsync(s->n_capped, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_nrm_window<true>, dim3(blocks_of(n_dirty)), dim3(kVoxBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  if (s->kn_max_nn == 0) return MC_OK;
  uint32_t n_capped = 0;
  if (int r = copy_back(c, &n_capped, s->n_capped, sizeof n_capped)) return r;
  if (n_capped > n_dirty) return fail(MC_ERR_STATE, "kept normals: %u capped voxels of %u dirty ones", n_capped, n_dirty);
  if (n_capped) {
    {
      TimedRegion tr(c, &s->ev[kKnCap], c->stream);
      hipLaunchKernelGGL(k_nrm_cap, dim3((n_capped + kNrmCapBlock - 1) / kNrmCapBlock), dim3(kNrmCapBlock), 0, c->stream, a);
    }
    HIPCHK(hipGetLastError());
  }
  return MC_OK;
}

int kept_refresh(mc_ctx* c, VoxState* s) {
  const int r = kept_refresh_run(c, s);
  if (r) s->kn_on = false;
  return r;
}

// whether the cloud keeps the normals of these parameters, compared as bits
bool kept_matches(const VoxState* s, double radius, int32_t max_nn) {
  return s->kn_on && s->M > 0 && std::memcmp(&s->kn_radius, &radius, sizeof radius) == 0 && s->kn_max_nn == max_nn;
}

// ---- the registration of a source against the cloud ------------------------------------------------------------------
// a 4 x 4 row-major pose argument (null: the identity) -> *T
int reg_pose(const double* m, const char* name, RegPose* T) {
  if (!m) {
    for (int i = 0; i < 9; ++i) T->R[i] = i % 4 == 0 ? 1.0 : 0.0;
    T->t[0] = T->t[1] = T->t[2] = 0.0;
    return MC_OK;
  }
  CHECK_ARG(m[12] == 0.0 && m[13] == 0.0 && m[14] == 0.0 && m[15] == 1.0, "%s: the last row must be 0, 0, 0, 1", name);
  pose_from_rows(m, T);
  CHECK_ARG(register_pose_ok(*T), "%s: the entries must be finite and the rotation orthonormal (|R^T R - I| <= 1e-6)", name);
  return MC_OK;
}

int reg_distance(const VoxState* s, double max_distance) {
  CHECK_ARG(std::isfinite(max_distance) && max_distance > 0.0, "max_distance must be finite and > 0 (got %g)", max_distance);
  return check_window(s, max_distance, "max_distance");
}

// the points of a batch (frame < 0: all of them, as one body) or of device rows as a source
int reg_source_batch(mc_ctx* c, const mc_batch* in, int32_t frame, RegSrc* src) {
  CHECK_ARG(in, "the source batch is NULL");
  CHECK_ARG(in->ctx == c, "batch belongs to another context");
  CHECK_ARG(frame >= -1 && frame < in->F, "frame %d of a batch of %d frames", frame, in->F);
  *src = {};
  src->cols = in->d_cols; src->C = in->C; src->F = in->F;
  src->poff = in->d_poff; src->doff = in->d_doff;
  src->first = frame < 0 ? 0 : in->doff[frame];
  src->n = frame < 0 ? in->N : in->counts[frame];
  CHECK_ARG(src->n >= 1, "the source is empty");
  CHECK_ARG(src->n < ((int64_t)1 << 31), "%lld points: a source takes fewer than 2^31", (long long)src->n);
  return MC_OK;
}

int reg_source_rows(const double* d_rows, int64_t ld, int64_t n, RegSrc* src) {
  CHECK_ARG(ld >= 3, "source rows are x, y, z: ld >= 3; got %lld", (long long)ld);
  CHECK_ARG(n >= 1, "the source is empty");
  CHECK_ARG(n < ((int64_t)1 << 31), "%lld points: a source takes fewer than 2^31", (long long)n);
  CHECK_ARG(d_rows, "d_rows is NULL");
  *src = {};
  src->rows = d_rows; src->ld = ld; src->n = n;
  return MC_OK;
}

// what both kernels read of the live build (its centroids written), for a window of max_distance
int reg_args(mc_ctx* c, VoxState* s, const RegSrc& src, double max_distance, RegArgs* a) {
  *a = {};
  a->src = src;
  a->M = s->M;
  a->h = s->h;
  std::copy_n(s->o, 3, a->o);
  a->w = query_of(s, max_distance, 0);
  if (s->M == 0) return MC_OK;   // no table and no centroids: every point is without a pair
  if (int r = centroids(c, s)) return r;
  a->g = grid_of(s);
  return MC_OK;
}

template <bool BATCH>
int reg_correspond(mc_ctx* c, VoxState* s, const RegArgs& a) {
  {
    TimedRegion tr(c, &s->ev[kRgCorrespond], c->stream);
    hipLaunchKernelGGL(k_rg_correspond<BATCH>, dim3(blocks_of(a.src.n)), dim3(kVoxBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return MC_OK;
}

template <bool BATCH>
int nearest_run(mc_ctx* c, const RegSrc& src, double max_distance, const double* transform, int32_t* d_ids, double* d_dist2,
                const char* who) {
  VoxState* s;
  if (int r = live_build(c, who, &s)) return r;
  if (int r = reg_distance(s, max_distance)) return r;
  RegPose T;
  if (int r = reg_pose(transform, "transform", &T)) return r;
  CHECK_ARG(d_ids && d_dist2, "d_ids or d_dist2 is NULL");
  DeviceGuard g(c->device);
  RegArgs a;
  if (int r = reg_args(c, s, src, max_distance, &a)) return r;
  a.T = T;
  a.ids = d_ids;
  a.d2 = d_dist2;
  return reg_correspond<BATCH>(c, s, a);
}

template <bool BATCH>
int register_run(mc_ctx* c, const RegSrc& src, const mc_register_params* p, double* transformation, double* history,
                 int64_t* stats, const char* who) {
  VoxState* s;
  if (int r = live_build(c, who, &s)) return r;
  if (int r = reg_distance(s, p->max_distance)) return r;
  CHECK_ARG(p->max_iterations >= 1 && p->max_iterations <= kRegMaxIterations, "max_iterations must be in 1..%d (got %d)",
            kRegMaxIterations, p->max_iterations);
  CHECK_ARG(std::isfinite(p->tol_rotation) && p->tol_rotation >= 0.0 && std::isfinite(p->tol_translation) &&
                p->tol_translation >= 0.0,
            "tol_rotation and tol_translation must be finite and >= 0 (got %g, %g)", p->tol_rotation, p->tol_translation);
  RegPose T;
  if (int r = reg_pose(p->init, "init", &T)) return r;
  const int64_t N = src.n, M = s->M;
  stats[3] = N;
  DeviceGuard g(c->device);
  // the normals of the call, into the state's scratch (their own checks of the radius and of max_nn)
  // (kept normals of these very parameters are read where they are: no normals kernel runs)
  const bool kept = kept_matches(s, p->normals_radius, p->max_nn);
  if (!kept) {
    if (int r = ctx_reserve(c, s->rg_normals, 4 * (size_t)std::max<int64_t>(M, 1))) return r;
    if (int r = ctx_reserve(c, s->rg_counts, (size_t)std::max<int64_t>(M, 1))) return r;
    if (int r = normals_run(c, p->normals_radius, p->max_nn, nullptr, s->rg_normals, s->rg_counts, nullptr, who, true)) return r;
  }
  const int64_t L = plane_leaves(N);
  const size_t words = tree_words(kRegSums, L);
  if (int r = ctx_reserve(c, s->rg_ids, (size_t)N)) return r;
  if (int r = ctx_reserve(c, s->rg_tree, words + 1)) return r;   // the pair counter behind the last level
  RegArgs a;
  if (int r = reg_args(c, s, src, p->max_distance, &a)) return r;
  a.T = T;
  a.ids = s->rg_ids;
  a.normals = kept ? s->kn_normals : s->rg_normals;
  a.counts = kept ? s->kn_counts : s->rg_counts;
  a.out = s->rg_tree;
  a.pairs = reinterpret_cast<unsigned long long*>(s->rg_tree.get() + words);
  int64_t last = L / kVoxBlock;
  while (last >= kVoxBlock) last /= kVoxBlock;
  std::vector<double> top((size_t)kRegSums * last + 1);
  int status = kRegGoOn;
  int32_t it = 0;
  int64_t pairs = 0;
  while (status == kRegGoOn && it < p->max_iterations) {
    if (int r = reg_correspond<BATCH>(c, s, a)) return r;
    int64_t cnt = L / kVoxBlock;
    double* cur = s->rg_tree;
    {
      TimedRegion tr(c, &s->ev[kRgLeaves], c->stream);
      HIPCHK(hipMemsetAsync(a.pairs, 0, sizeof(unsigned long long), c->stream));
      hipLaunchKernelGGL(k_rg_leaves<BATCH>, dim3((uint32_t)cnt), dim3(kVoxBlock), 0, c->stream, a);
    }
    if (cnt >= kVoxBlock) {
      TimedRegion tr(c, &s->ev[kRgTree], c->stream);
      cur = tree_levels<kRegSums>(c, cur, &cnt);
    }
    HIPCHK(hipGetLastError());
    // the iteration's one copy: the last level's partials and the pair counter behind them
    if (int r = copy_back(c, top.data(), cur, top.size() * sizeof(double))) return r;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long found = 0;
    std::memcpy(&found, &top[(size_t)kRegSums * cnt], sizeof found);
    if ((int64_t)found > N) return fail(MC_ERR_STATE, "voxel register: %llu pairs of %lld points", found, (long long)N);
    pairs = (int64_t)found;
    double sums[kRegSums];
    tree_top(top.data(), cnt, kRegSums, sums);
    status = register_step(sums, pairs, p->tol_rotation, p->tol_translation, &a.T, history + (size_t)kRegHistory * it);
    ++it;
    if (c->timing) {
      s->rg_solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      ++s->rg_solve_n;
    }
  }
  if (status == kRegGoOn) status = kRegMaxIter;
  pose_to_rows(a.T, transformation);
  stats[0] = pairs;
  stats[1] = it;
  stats[2] = status;
  return MC_OK;
}

// ---- the frames of a batch registered together -----------------------------------------------------------------------
constexpr int64_t kRegFramesHistoryRows = (int64_t)1 << 22;   // F x max_iterations at most: 256 MB of history
constexpr int kRegFramesLevels = 3;                            // fewer than 2^31 points: 2^23 partials, 2^15, 2^7

// Every frame of `in` registered on its own (include/mcdeskew.h mc_voxel_register_frames): per iteration the step
// over every live frame's points, the further levels of the frames that have them, the solve of every live frame,
// and one synchronisation with one word copied: the frames still live.  inits: F x 16, or null: p->init for all
int register_frames_run(mc_ctx* c, const mc_batch* in, const mc_register_params* p, const double* inits, double* transformations,
                        double* history, int64_t* stats, const char* who) {
  VoxState* s;
  if (int r = live_build(c, who, &s)) return r;
  if (int r = reg_distance(s, p->max_distance)) return r;
  CHECK_ARG(p->max_iterations >= 1 && p->max_iterations <= kRegMaxIterations, "max_iterations must be in 1..%d (got %d)",
            kRegMaxIterations, p->max_iterations);
  CHECK_ARG(std::isfinite(p->tol_rotation) && p->tol_rotation >= 0.0 && std::isfinite(p->tol_translation) &&
                p->tol_translation >= 0.0,
            "tol_rotation and tol_translation must be finite and >= 0 (got %g, %g)", p->tol_rotation, p->tol_translation);
  const int32_t F = in->F;
  CHECK_ARG((int64_t)F * p->max_iterations <= kRegFramesHistoryRows,
            "%d frames x max_iterations %d is more than %lld history rows (256 MB): lower max_iterations", F, p->max_iterations,
            (long long)kRegFramesHistoryRows);
  // the records, the block maps of the levels and the words of the trees, on the host
  std::vector<RegFrame> fr((size_t)F);
  std::vector<int64_t> map((size_t)kRegFramesLevels * (F + 1), 0);
  int64_t words = 0;
  for (int32_t f = 0; f < F; ++f) {
    const int64_t n = in->counts[f];
    CHECK_ARG(n < ((int64_t)1 << 31), "frame %d: %lld points: a source takes fewer than 2^31", f, (long long)n);
    RegPose T;
    char name[48] = "init";
    if (inits) std::snprintf(name, sizeof name, "init of frame %d", f);
    if (int r = reg_pose(inits ? inits + 16 * (size_t)f : p->init, name, &T)) return r;
    words += register_frame_init(&fr[f], T, n, words);
    int64_t cnt = fr[f].blocks;
    for (int l = 0; l < kRegFramesLevels; ++l) {
      int64_t* off = map.data() + (size_t)l * (F + 1);
      off[f + 1] = off[f] + cnt;
      cnt = cnt >= kRegBlock ? cnt / kRegBlock : 0;     // the workgroups of the next level; none below 256 partials
    }
    stats[4 * f + 3] = n;
  }
  const int64_t* top_map = map.data();
  CHECK_ARG(top_map[F] < ((int64_t)1 << 31), "%lld workgroups of 256 points: a launch takes fewer than 2^31", (long long)top_map[F]);
  const int64_t M = s->M;
  DeviceGuard g(c->device);
  // the normals of the call, once for all frames
  const bool kept = kept_matches(s, p->normals_radius, p->max_nn);   // as register_run
  if (!kept) {
    if (int r = ctx_reserve(c, s->rg_normals, 4 * (size_t)std::max<int64_t>(M, 1))) return r;
    if (int r = ctx_reserve(c, s->rg_counts, (size_t)std::max<int64_t>(M, 1))) return r;
    if (int r = normals_run(c, p->normals_radius, p->max_nn, nullptr, s->rg_normals, s->rg_counts, nullptr, who, true, kRfNormals)) return r;
  }
  const size_t rows = (size_t)F * p->max_iterations;
  int32_t live = 0;
  for (int32_t f = 0; f < F; ++f) live += fr[f].status == kRegGoOn;
  if (live > 0) {
    if (int r = ctx_reserve(c, s->rf_frames, (size_t)F)) return r;
    if (int r = ctx_reserve(c, s->rf_map, map.size())) return r;
    if (int r = ctx_reserve(c, s->rf_tree, (size_t)words)) return r;
    if (int r = ctx_reserve(c, s->rf_history, (size_t)kRegHistory * rows)) return r;
    if (!s->rf_live) if (int r = s->rf_live.alloc(1)) return r;
    RegFramesArgs a = {};
    a.cols = in->d_cols; a.C = in->C; a.F = F;
    a.poff = in->d_poff;
    a.fr = s->rf_frames;
    a.M = M;
    a.h = s->h;
    std::copy_n(s->o, 3, a.o);
    a.w = query_of(s, p->max_distance, 0);
    if (M > 0) {
      if (int r = centroids(c, s)) return r;
      a.g = grid_of(s);
    }
    a.normals = kept ? s->kn_normals : s->rg_normals;
    a.counts = kept ? s->kn_counts : s->rg_counts;
    a.tree = s->rf_tree;
    a.max_iterations = p->max_iterations;
    a.tol_rotation = p->tol_rotation; a.tol_translation = p->tol_translation;
    a.history = s->rf_history;
    a.live = s->rf_live;
    HIPCHK(hipMemcpyAsync(s->rf_frames, fr.data(), fr.size() * sizeof(RegFrame), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->rf_map, map.data(), map.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->rf_tree, 0, (size_t)words * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(s->rf_history, 0, (size_t)kRegHistory * rows * sizeof(double), c->stream));
    for (int32_t it = 0; live > 0 && it < p->max_iterations; ++it) {
      {
        TimedRegion tr(c, &s->ev[kRfStep], c->stream);
        HIPCHK(hipMemsetAsync(s->rf_live, 0, sizeof(uint32_t), c->stream));
        a.boff = s->rf_map.get();
        hipLaunchKernelGGL(k_rg_frames_step, dim3((uint32_t)top_map[F]), dim3(kVoxBlock), 0, c->stream, a);
      }
      for (int l = 1; l < kRegFramesLevels; ++l) {
        const int64_t blocks = map[(size_t)l * (F + 1) + F];
        if (blocks == 0) break;
        TimedRegion tr(c, &s->ev[kRfTree], c->stream);
        a.boff = s->rf_map.get() + (size_t)l * (F + 1);
        a.level = l + 1;
        hipLaunchKernelGGL(k_rg_frames_tree, dim3((uint32_t)blocks), dim3(kVoxBlock), 0, c->stream, a);
      }
      {
        TimedRegion tr(c, &s->ev[kRfSolve], c->stream);
        hipLaunchKernelGGL(k_rg_frames_solve, dim3((uint32_t)F), dim3(kVoxBlock), 0, c->stream, a);
      }
      HIPCHK(hipGetLastError());
      // the iteration's one synchronisation and its one word
      uint32_t on = 0;
      if (int r = copy_back(c, &on, s->rf_live, sizeof on)) return r;
      if ((int64_t)on > live) return fail(MC_ERR_STATE, "voxel register frames: %u live frames of %d", on, live);
      live = (int32_t)on;
    }
    // the call's one copy of the records and of the history
    HIPCHK(hipMemcpyAsync(fr.data(), s->rf_frames, fr.size() * sizeof(RegFrame), hipMemcpyDeviceToHost, c->stream));
    if (int r = copy_back(c, history, s->rf_history, (size_t)kRegHistory * rows * sizeof(double))) return r;
  } else {
    std::fill_n(history, (size_t)kRegHistory * rows, 0.0);
  }
  for (int32_t f = 0; f < F; ++f) {
    const RegFrame& r = fr[f];
    if (r.pairs < 0 || r.pairs > r.n || r.iterations < 0 || r.iterations > p->max_iterations || r.status < 0 || r.status > kRegEmpty)
      return fail(MC_ERR_STATE, "voxel register frames: frame %d ended with %lld pairs of %lld points, %d iterations, status %d", f,
                  (long long)r.pairs, (long long)r.n, r.iterations, r.status);
    pose_to_rows(r.T, transformations + 16 * (size_t)f);
    stats[4 * f + 0] = r.pairs;
    stats[4 * f + 1] = r.iterations;
    stats[4 * f + 2] = r.status;
  }
  return MC_OK;
}

// ---- the rays of a source through the cloud ---------------------------------------------------------------------------
// a: the source and the sensor positions set; the walk of every ray (include/mcdeskew.h mc_voxel_rays_*): one clear,
// one launch, one synchronisation with the two counters copied
template <bool BATCH>
int rays_run(mc_ctx* c, VoxState* s, RaysArgs a, int64_t n, int64_t lanes, int32_t guard, int32_t max_steps, int32_t* d_passed,
             int32_t* d_ended, int32_t* d_through, int64_t* stats) {
  const int64_t M = s->M;
  a.G = {};
  a.G.M = M;
  a.G.h = s->h;
  std::copy_n(s->o, 3, a.G.o);
  if (M > 0) a.G.g = grid_of(s);   // the centroids are not read
  a.guard = guard;
  a.max_steps = max_steps;
  a.passed = d_passed; a.ended = d_ended; a.through = d_through;
  if (int r = ctx_reserve(c, s->ry_meta, (size_t)kRaysMeta)) return r;
  a.meta = s->ry_meta;
  {
    TimedRegion tr(c, &s->ev[kRyClear], c->stream);
    if (M > 0) {
      HIPCHK(hipMemsetAsync(d_passed, 0, (size_t)M * sizeof(int32_t), c->stream));
      HIPCHK(hipMemsetAsync(d_ended, 0, (size_t)M * sizeof(int32_t), c->stream));
    }
    HIPCHK(hipMemsetAsync(s->ry_meta, 0, kRaysMeta * sizeof(unsigned long long), c->stream));
  }
  {
    TimedRegion tr(c, &s->ev[kRyWalk], c->stream);
    hipLaunchKernelGGL(k_rays_walk<BATCH>, dim3(blocks_of(lanes)), dim3(kVoxBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  unsigned long long meta[kRaysMeta] = {0, 0};
  if (int r = copy_back(c, meta, s->ry_meta, sizeof meta)) return r;
  if ((int64_t)meta[kRaysMetaSkipped] > n || meta[kRaysMetaSteps] > (unsigned long long)n * (unsigned long long)max_steps)
    return fail(MC_ERR_STATE, "voxel rays: %llu skipped and %llu steps of %lld rays of at most %d steps", meta[kRaysMetaSkipped],
                meta[kRaysMetaSteps], (long long)n, max_steps);
  stats[0] = n;
  stats[1] = (int64_t)meta[kRaysMetaSkipped];
  stats[2] = (int64_t)meta[kRaysMetaSteps];
  stats[3] = 0;
  return MC_OK;
}

// what both entry points check of their plain arguments, and the state of the live build
int rays_checks(mc_ctx* c, int32_t guard, int32_t max_steps, const int32_t* d_passed, const int32_t* d_ended,
                const int32_t* d_through, const char* who, VoxState** s) {
  CHECK_ARG(guard >= 0 && guard <= kRaysMaxGuard, "guard must be in 0..%d (got %d)", kRaysMaxGuard, guard);
  CHECK_ARG(max_steps >= 1 && max_steps <= kRaysMaxSteps, "max_steps must be in 1..%d (got %d)", kRaysMaxSteps, max_steps);
  CHECK_ARG(d_through, "d_through is NULL");
  if (int r = live_build(c, who, s)) return r;
  CHECK_ARG((*s)->M == 0 || (d_passed && d_ended), "d_passed or d_ended is NULL");
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_voxel_build_batch(mc_ctx* c, const mc_batch* in, double voxel, const double* origin, int64_t* n_voxels,
                         int32_t* bad_frame, int64_t* bad_index) {
  if (bad_frame) *bad_frame = -1;
  if (bad_index) *bad_index = -1;
  CHECK_ARG(c && in && n_voxels, "NULL argument");
  CHECK_ARG(in->ctx == c, "batch belongs to another context");
  if (int r = check_grid(voxel, origin)) return r;
  CHECK_ARG(in->N < ((int64_t)1 << 31), "%lld points: the voxel filter takes fewer than 2^31", (long long)in->N);
  DeviceGuard g(c->device);
  VoxSrc src = batch_source(in);
  src.h = voxel;
  std::copy_n(origin, 3, src.o);
  int64_t bad = -1;
  const int r = build<true>(c, src, in->N, in->P / 4, n_voxels, &bad);
  if (bad >= 0) {
    const int32_t f = frame_of(in, bad);
    if (bad_frame) *bad_frame = f;
    if (bad_index) *bad_index = bad - in->doff[f];
    return fail(MC_ERR_INVALID, "frame %d, point %lld (the lowest refused): %s", f, (long long)(bad - in->doff[f]), kRefused);
  }
  return r;
}

int mc_voxel_build_f64(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, double voxel, const double* origin,
                       int64_t* n_voxels, int64_t* bad_row) {
  if (bad_row) *bad_row = -1;
  CHECK_ARG(c && n_voxels, "NULL argument");
  CHECK_ARG(ld >= 4, "voxel rows are x, y, z, intensity: ld >= 4; got %lld", (long long)ld);
  CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "%lld points: the voxel filter takes 0 to 2^31 - 1", (long long)n);
  CHECK_ARG(n == 0 || d_rows, "d_rows is NULL");
  if (int r = check_grid(voxel, origin)) return r;
  DeviceGuard g(c->device);
  VoxSrc src = {};
  src.rows = d_rows; src.ld = ld; src.n = n;
  src.h = voxel;
  std::copy_n(origin, 3, src.o);
  int64_t bad = -1;
  const int r = build<false>(c, src, n, n, n_voxels, &bad);
  if (bad >= 0) {
    if (bad_row) *bad_row = bad;
    return fail(MC_ERR_INVALID, "row %lld (the lowest refused): %s", (long long)bad, kRefused);
  }
  return r;
}

int mc_voxel_emit_batch(mc_ctx* c, mc_batch* out) {
  CHECK_ARG(c && out, "NULL argument");
  CHECK_ARG(out->ctx == c, "batch belongs to another context");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_emit_batch", &s)) return r;
  CHECK_ARG(out->F == 1 && out->N == s->M, "the out batch must be one frame of exactly %lld points (it has %d frames, %lld points)",
            (long long)s->M, out->F, (long long)out->N);
  DeviceGuard g(c->device);
  VoxOut a = out_of(s);
  a.cols = out->d_cols;
  a.C = out->C;
  if (int r = emit(c, s, a, true, out->P)) return r;
  return mcimpl::batch_columns_written(out, mcimpl::kWroteAllQueued);
}

int mc_voxel_emit_f64(mc_ctx* c, double* d_rows, int32_t* d_counts, int32_t* d_keys) {
  CHECK_ARG(c, "ctx is NULL");
  CHECK_ARG(((uintptr_t)d_rows & 15) == 0, "d_rows must be 16-byte aligned");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_emit_f64", &s)) return r;
  if (!d_rows && !d_counts && !d_keys) return MC_OK;
  DeviceGuard g(c->device);
  VoxOut a = out_of(s);
  a.rows = d_rows;
  a.counts = d_counts;
  a.keys_out = d_keys;
  return emit(c, s, a, false, 0);
}

int mc_voxel_insert_batch(mc_ctx* c, const mc_batch* in, int64_t* n_new, int32_t* bad_frame, int64_t* bad_index) {
  if (bad_frame) *bad_frame = -1;
  if (bad_index) *bad_index = -1;
  if (n_new) *n_new = 0;
  CHECK_ARG(c && in && n_new, "NULL argument");
  CHECK_ARG(in->ctx == c, "batch belongs to another context");
  CHECK_ARG(in->N < kVoxelPointsEnd, "%lld points: a cloud takes fewer than 2^31 in all", (long long)in->N);
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_insert_batch", &s)) return r;
  DeviceGuard g(c->device);
  int64_t bad = -1;
  const int r = insert<kVoxBatch>(c, s, batch_source(in), in->N, in->P / 4, in->N, n_new, &bad);
  if (bad >= 0) {
    const int32_t f = frame_of(in, bad);
    if (bad_frame) *bad_frame = f;
    if (bad_index) *bad_index = bad - in->doff[f];
    return fail(MC_ERR_INVALID, "frame %d, point %lld (the lowest refused; the cloud is unchanged): %s", f,
                (long long)(bad - in->doff[f]), kRefused);
  }
  return r;
}

int mc_voxel_insert_f64(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, int64_t* n_new, int64_t* bad_row) {
  if (bad_row) *bad_row = -1;
  if (n_new) *n_new = 0;
  CHECK_ARG(c && n_new, "NULL argument");
  CHECK_ARG(ld >= 4, "voxel rows are x, y, z, intensity: ld >= 4; got %lld", (long long)ld);
  CHECK_ARG(n >= 0 && n < kVoxelPointsEnd, "%lld points: a cloud takes 0 to 2^31 - 1 in all", (long long)n);
  CHECK_ARG(n == 0 || d_rows, "d_rows is NULL");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_insert_f64", &s)) return r;
  DeviceGuard g(c->device);
  VoxSrc src = {};
  src.rows = d_rows; src.ld = ld; src.n = n;
  int64_t bad = -1;
  const int r = insert<kVoxRows>(c, s, src, n, n, n, n_new, &bad);
  if (bad >= 0) {
    if (bad_row) *bad_row = bad;
    return fail(MC_ERR_INVALID, "row %lld (the lowest refused; the cloud is unchanged): %s", (long long)bad, kRefused);
  }
  return r;
}

int mc_voxel_merge_sums(mc_ctx* c, const int32_t* d_keys, const int32_t* d_counts, const int64_t* d_sums, int64_t m,
                        int64_t* n_new, int64_t* bad_record) {
  if (bad_record) *bad_record = -1;
  if (n_new) *n_new = 0;
  CHECK_ARG(c && n_new, "NULL argument");
  CHECK_ARG(m >= 0 && m < kVoxelPointsEnd, "%lld records: a merge takes 0 to 2^31 - 1", (long long)m);
  CHECK_ARG(m == 0 || (d_keys && d_counts && d_sums), "d_keys, d_counts or d_sums is NULL");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_merge_sums", &s)) return r;
  DeviceGuard g(c->device);
  VoxRecSrc src = {};
  src.keys = d_keys; src.counts = d_counts; src.sums = reinterpret_cast<const long long*>(d_sums);
  src.n = m;
  int64_t bad = -1;
  const int r = insert<kVoxRecords>(c, s, src, m, m, -1, n_new, &bad);
  if (bad >= 0) {
    if (bad_record) *bad_record = bad;
    return fail(MC_ERR_INVALID,
                "record %lld (the lowest refused; the cloud is unchanged): a count below 1, a key outside [-2^20, 2^20), a "
                "coordinate sum outside 0 .. count * 2^32 or an intensity sum beyond +-count * 2^32", (long long)bad);
  }
  return r;
}

int mc_voxel_emit_sums(mc_ctx* c, int64_t* d_sums) {
  CHECK_ARG(c, "ctx is NULL");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_emit_sums", &s)) return r;
  if (s->M == 0) return MC_OK;
  CHECK_ARG(d_sums, "d_sums is NULL");
  DeviceGuard g(c->device);
  HIPCHK(hipMemcpyAsync(d_sums, s->sums, kVoxRec * (size_t)s->M * sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
  return MC_OK;
}

int mc_voxel_points(mc_ctx* c, int64_t* n_points) {
  CHECK_ARG(c && n_points, "NULL argument");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_points", &s)) return r;
  *n_points = s->N;
  return MC_OK;
}

int mc_voxel_table(mc_ctx* c, int64_t* slots, int64_t* growths) {
  CHECK_ARG(c, "ctx is NULL");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_table", &s)) return r;
  if (slots) *slots = s->log2cap ? (int64_t)1 << s->log2cap : 0;
  if (growths) *growths = s->growths;
  return MC_OK;
}

int mc_timing_read_voxel_insert(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kInsertPhases, ms_phase, launches);
}

int mc_voxel_remove(mc_ctx* c, const uint8_t* d_mask, int64_t* n_removed) {
  if (n_removed) *n_removed = 0;
  CHECK_ARG(c && n_removed, "NULL argument");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_remove", &s)) return r;
  s->kn_last = 0;   // an all-False mask recomputes no kept row
  if (s->M == 0) return MC_OK;
  CHECK_ARG(d_mask, "d_mask is NULL");
  DeviceGuard g(c->device);
  if (int r = keep_flags(c, s, d_mask)) return r;
  return keep_voxels(c, s, n_removed);
}

int mc_voxel_subtract_batch(mc_ctx* c, const mc_batch* in, int64_t* n_emptied, int32_t* bad_frame, int64_t* bad_index, int32_t* why) {
  if (bad_frame) *bad_frame = -1;
  if (bad_index) *bad_index = -1;
  if (n_emptied) *n_emptied = 0;
  if (why) *why = MC_VOXEL_SUB_OK;
  CHECK_ARG(c && in && n_emptied, "NULL argument");
  CHECK_ARG(in->ctx == c, "batch belongs to another context");
  CHECK_ARG(in->N < kVoxelPointsEnd, "%lld points: a cloud holds fewer than 2^31 in all", (long long)in->N);
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_subtract_batch", &s)) return r;
  DeviceGuard g(c->device);
  SubRefusal ref;
  const int r = subtract<kVoxBatch>(c, s, batch_source(in), in->N, in->P / 4, in->N, n_emptied, &ref);
  if (why) *why = ref.why;
  if (ref.item >= 0) {
    const int32_t f = frame_of(in, ref.item);
    if (bad_frame) *bad_frame = f;
    if (bad_index) *bad_index = ref.item - in->doff[f];
    char item[64];
    std::snprintf(item, sizeof item, "frame %d, point %lld", f, (long long)(ref.item - in->doff[f]));
    return subtract_refused(item, ref, kRefused);
  }
  return r;
}

int mc_voxel_subtract_f64(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, int64_t* n_emptied, int64_t* bad_row, int32_t* why) {
  if (bad_row) *bad_row = -1;
  if (n_emptied) *n_emptied = 0;
  if (why) *why = MC_VOXEL_SUB_OK;
  CHECK_ARG(c && n_emptied, "NULL argument");
  CHECK_ARG(ld >= 4, "voxel rows are x, y, z, intensity: ld >= 4; got %lld", (long long)ld);
  CHECK_ARG(n >= 0 && n < kVoxelPointsEnd, "%lld points: a cloud holds 0 to 2^31 - 1 in all", (long long)n);
  CHECK_ARG(n == 0 || d_rows, "d_rows is NULL");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_subtract_f64", &s)) return r;
  DeviceGuard g(c->device);
  VoxSrc src = {};
  src.rows = d_rows; src.ld = ld; src.n = n;
  SubRefusal ref;
  const int r = subtract<kVoxRows>(c, s, src, n, n, n, n_emptied, &ref);
  if (why) *why = ref.why;
  if (ref.item >= 0) {
    if (bad_row) *bad_row = ref.item;
    char item[48];
    std::snprintf(item, sizeof item, "row %lld", (long long)ref.item);
    return subtract_refused(item, ref, kRefused);
  }
  return r;
}

int mc_voxel_subtract_sums(mc_ctx* c, const int32_t* d_keys, const int32_t* d_counts, const int64_t* d_sums, int64_t m,
                           int64_t* n_emptied, int64_t* bad_record, int32_t* why) {
  if (bad_record) *bad_record = -1;
  if (n_emptied) *n_emptied = 0;
  if (why) *why = MC_VOXEL_SUB_OK;
  CHECK_ARG(c && n_emptied, "NULL argument");
  CHECK_ARG(m >= 0 && m < kVoxelPointsEnd, "%lld records: a subtraction takes 0 to 2^31 - 1", (long long)m);
  CHECK_ARG(m == 0 || (d_keys && d_counts && d_sums), "d_keys, d_counts or d_sums is NULL");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_subtract_sums", &s)) return r;
  DeviceGuard g(c->device);
  VoxRecSrc src = {};
  src.keys = d_keys; src.counts = d_counts; src.sums = reinterpret_cast<const long long*>(d_sums);
  src.n = m;
  SubRefusal ref;
  const int r = subtract<kVoxRecords>(c, s, src, m, m, -1, n_emptied, &ref);
  if (why) *why = ref.why;
  if (ref.item >= 0) {
    if (bad_record) *bad_record = ref.item;
    char item[48];
    std::snprintf(item, sizeof item, "record %lld", (long long)ref.item);
    return subtract_refused(item, ref,
                            "a count below 1, a key outside [-2^20, 2^20), a coordinate sum outside 0 .. count * 2^32 or an intensity "
                            "sum beyond +-count * 2^32");
  }
  return r;
}

int mc_timing_read_voxel_remove(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kRemovePhases, ms_phase, launches);
}

int mc_timing_read_voxel(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kFilterPhases, ms_phase, launches);
}

int mc_voxel_normals(mc_ctx* c, double radius, int32_t max_nn, const double* viewpoint, double* d_normals,
                     int32_t* d_counts, double* d_cov) {
  CHECK_ARG(c, "ctx is NULL");
  return normals_run(c, radius, max_nn, viewpoint, d_normals, d_counts, d_cov, "mc_voxel_normals", false);
}

int mc_timing_read_normals(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kNormalsPhases, ms_phase, launches);
}

int mc_voxel_keep_normals(mc_ctx* c, double radius, int32_t max_nn) {
  CHECK_ARG(c, "ctx is NULL");
  if (int r = normals_checks(radius, max_nn, nullptr)) return r;
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_keep_normals", &s)) return r;
  if (int r = check_window(s, radius, "radius")) return r;
  DeviceGuard g(c->device);
  s->kn_on = false;   // what was kept is replaced; a failure from here leaves none kept
  s->kn_last = 0;
  if (int r = kept_reserve(c, s, 0, s->M)) return r;
  s->kn_epoch = 0;    // every stamp is 0 again
  if (int r = normals_run(c, radius, max_nn, nullptr, s->kn_normals, s->kn_counts, nullptr, "mc_voxel_keep_normals", false)) return r;
  s->cent_current = true;   // of a cloud without voxels too
  s->kn_radius = radius;
  s->kn_max_nn = max_nn;
  ++s->kn_full;
  s->kn_on = true;
  return MC_OK;
}

// the state of a live build that keeps normals, for the entry point `who`
static int kept_state(mc_ctx* c, const char* who, VoxState** s) {
  if (int r = live_build(c, who, s)) return r;
  if (!(*s)->kn_on) return fail(MC_ERR_STATE, "%s: the cloud keeps no normals (mc_voxel_keep_normals)", who);
  return MC_OK;
}

int mc_voxel_kept_normals(mc_ctx* c, double* d_normals, int32_t* d_counts) {
  CHECK_ARG(c, "ctx is NULL");
  VoxState* s;
  if (int r = kept_state(c, "mc_voxel_kept_normals", &s)) return r;
  if (s->M == 0) return MC_OK;
  DeviceGuard g(c->device);
  if (d_normals) HIPCHK(hipMemcpyAsync(d_normals, s->kn_normals, 4 * (size_t)s->M * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (d_counts) HIPCHK(hipMemcpyAsync(d_counts, s->kn_counts, (size_t)s->M * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
  return MC_OK;
}

int mc_voxel_kept_info(mc_ctx* c, double* radius, int32_t* max_nn, int64_t* counters) {
  CHECK_ARG(c, "ctx is NULL");
  VoxState* s;
  if (int r = kept_state(c, "mc_voxel_kept_info", &s)) return r;
  if (radius) *radius = s->kn_radius;
  if (max_nn) *max_nn = s->kn_max_nn;
  if (counters) {
    counters[0] = s->kn_full;
    counters[1] = s->kn_last;
    counters[2] = s->kn_total;
  }
  return MC_OK;
}

int mc_voxel_drop_normals(mc_ctx* c) {
  CHECK_ARG(c, "ctx is NULL");
  VoxState* s = state_of(c, false);
  if (!s) return MC_OK;
  DeviceGuard g(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));   // the blocks are idle when they go back
  kept_free(s);
  return MC_OK;
}

int mc_timing_read_kept_normals(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kKeptPhases, ms_phase, launches);
}

int mc_voxel_clusters(mc_ctx* c, double eps, int32_t min_points, int32_t weighted, int32_t* d_labels, int32_t* d_density,
                      int64_t* n_clusters) {
  if (n_clusters) *n_clusters = 0;
  CHECK_ARG(c, "ctx is NULL");
  CHECK_ARG(std::isfinite(eps) && eps > 0.0, "eps must be finite and > 0 (got %g)", eps);
  CHECK_ARG(min_points >= 1, "min_points must be >= 1 (got %d)", min_points);
  CHECK_ARG(weighted == 0 || weighted == 1, "weighted must be 0 or 1 (got %d)", weighted);
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_clusters", &s)) return r;
  if (int r = check_window(s, eps, "eps")) return r;
  const int64_t M = s->M;
  CHECK_ARG(M == 0 || d_labels, "d_labels is NULL");
  s->cl_current = false;   // a refused call leaves the last clustering; one that starts replaces it
  s->cl_K = 0;
  if (M == 0) { s->cl_current = true; return MC_OK; }
  DeviceGuard g(c->device);
  const uint32_t blocks = blocks_of(M);
  if (int r = centroids(c, s)) return r;
  if (int r = ctx_reserve(c, s->cl_parent, (size_t)M)) return r;
  if (int r = ctx_reserve(c, s->cl_label, (size_t)M)) return r;
  if (int r = ctx_reserve(c, s->cl_chunk, (size_t)blocks)) return r;
  if (!s->cl_meta) if (int r = s->cl_meta.alloc(2)) return r;
  ClusterArgs a = {};
  a.g = grid_of(s);
  a.vslot = s->vslot;
  a.cnt = s->cnt;
  a.M = M;
  a.q = cluster_query(window_cells(s, eps), eps * eps);
  a.min_points = min_points;
  a.weighted = weighted;
  a.parent = s->cl_parent; a.label = s->cl_label; a.chunk = s->cl_chunk;
  a.labels_out = d_labels; a.density_out = d_density;
  const dim3 blk(kVoxBlock), grid(blocks);
  {
    TimedRegion tr(c, &s->ev[kClDensity], c->stream);
    hipLaunchKernelGGL(k_cl_density, grid, blk, 0, c->stream, a);
  }
  {
    TimedRegion tr(c, &s->ev[kClUnion], c->stream);
    hipLaunchKernelGGL(k_cl_union, grid, blk, 0, c->stream, a);
  }
  {
    TimedRegion tr(c, &s->ev[kClLabel], c->stream);
    hipLaunchKernelGGL(k_cl_label, grid, blk, 0, c->stream, a);
  }
  {
    TimedRegion tr(c, &s->ev[kClNumber], c->stream);
    hipLaunchKernelGGL(k_cl_flag, grid, blk, 0, c->stream, a);
    scan_counts(c, s->cl_chunk, blocks, s->cl_meta);
    hipLaunchKernelGGL(k_cl_rank, grid, blk, 0, c->stream, a);
    hipLaunchKernelGGL(k_cl_number, grid, blk, 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  // the one synchronisation: K
  uint32_t meta[2] = {0, 0};
  if (int r = copy_back(c, meta, s->cl_meta, sizeof meta)) return r;
  if ((int64_t)meta[1] > M) return fail(MC_ERR_STATE, "voxel clusters: %u clusters of %lld voxels", meta[1], (long long)M);
  s->cl_K = (int64_t)meta[1];
  s->cl_current = true;
  if (n_clusters) *n_clusters = s->cl_K;
  return MC_OK;
}

int mc_voxel_cluster_stats(mc_ctx* c, int32_t* d_voxels, int64_t* d_points, int32_t* d_cell_min, int32_t* d_cell_max) {
  CHECK_ARG(c, "ctx is NULL");
  VoxState* s = state_of(c, false);
  if (!s || !s->built || !s->cl_current)
    return fail(MC_ERR_STATE, "mc_voxel_cluster_stats needs a successful mc_voxel_clusters of the live build first");
  const int64_t K = s->cl_K;
  if (K == 0 || (!d_voxels && !d_points && !d_cell_min && !d_cell_max)) return MC_OK;
  DeviceGuard g(c->device);
  ClusterStatsArgs a = {};
  a.keys = s->keys; a.vslot = s->vslot; a.cnt = s->cnt; a.label = s->cl_label;
  a.M = s->M;
  a.voxels = d_voxels;
  a.points = reinterpret_cast<long long*>(d_points);
  a.cell_min = d_cell_min; a.cell_max = d_cell_max;
  {
    TimedRegion tr(c, &s->ev[kClStats], c->stream);
    // every cluster holds a voxel, so no start value survives: 0x7F7F7F7F is above and 0x80808080 below any key
    if (d_voxels) HIPCHK(hipMemsetAsync(d_voxels, 0, (size_t)K * sizeof(int32_t), c->stream));
    if (d_points) HIPCHK(hipMemsetAsync(d_points, 0, (size_t)K * sizeof(int64_t), c->stream));
    if (d_cell_min) HIPCHK(hipMemsetAsync(d_cell_min, 0x7F, (size_t)K * 3 * sizeof(int32_t), c->stream));
    if (d_cell_max) HIPCHK(hipMemsetAsync(d_cell_max, 0x80, (size_t)K * 3 * sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(k_cl_stats, dim3(blocks_of(s->M)), dim3(kVoxBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return MC_OK;
}

int mc_timing_read_clusters(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kClPhases, ms_phase, launches);
}

int mc_voxel_plane_chunk(void) { return kPlaneChunk; }

int mc_voxel_plane(mc_ctx* c, double distance, int32_t num_iterations, uint64_t seed, int32_t refine, const uint8_t* d_among,
                   uint8_t* d_inliers, double* model, double* cov, int32_t* samples, int64_t* stats) {
  if (model) std::fill_n(model, 4, 0.0);
  if (cov) std::fill_n(cov, 6, 0.0);
  if (samples) std::fill_n(samples, 3, -1);
  if (stats) { stats[0] = -1; stats[1] = stats[2] = stats[3] = 0; }
  CHECK_ARG(c && model && samples && stats, "NULL argument");
  CHECK_ARG(std::isfinite(distance) && distance > 0.0, "distance must be finite and > 0 (got %g)", distance);
  CHECK_ARG(num_iterations >= 1 && num_iterations <= kPlaneMaxIterations, "num_iterations must be in 1..%d (got %d)",
            kPlaneMaxIterations, num_iterations);
  CHECK_ARG(refine == 0 || refine == 1, "refine must be 0 or 1 (got %d)", refine);
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_plane", &s)) return r;
  const int64_t M = s->M;
  CHECK_ARG(M >= 3, "a plane needs three candidate voxels (the cloud has %lld)", (long long)M);
  DeviceGuard g(c->device);
  const int32_t K = num_iterations;
  if (int r = centroids(c, s)) return r;
  int64_t n = M;
  if (d_among) {
    if (int r = compact(c, s, d_among, kPlCompact, &n)) return r;
    CHECK_ARG(n >= 3, "a plane needs three candidate voxels (the mask has %lld)", (long long)n);
  }
  if (int r = ctx_reserve(c, s->pl_hyp, (size_t)kPlaneHyp * K)) return r;
  if (int r = ctx_reserve(c, s->pl_samples, (size_t)3 * K)) return r;
  if (int r = ctx_reserve(c, s->pl_score, (size_t)K)) return r;
  if (int r = ctx_reserve(c, s->pl_mask, (size_t)M)) return r;
  if (!s->pl_count) if (int r = s->pl_count.alloc(1)) return r;
  {
    PlaneSampleArgs a = {};
    a.cent = s->cent;
    a.ids = d_among ? s->pl_ids.get() : nullptr;
    a.n = n;
    a.seed = seed;
    a.K = K;
    a.tt = distance * distance;
    a.hyp = s->pl_hyp; a.samples = s->pl_samples;
    TimedRegion tr(c, &s->ev[kPlSample], c->stream);
    hipLaunchKernelGGL(k_pl_sample, dim3(blocks_of(K)), dim3(kVoxBlock), 0, c->stream, a);
  }
  {
    const int64_t tiles = (M + kPlaneTile - 1) / kPlaneTile;
    const dim3 grid((uint32_t)std::min<int64_t>(tiles, kPlaneScoreGrid));
    TimedRegion tr(c, &s->ev[kPlScore], c->stream);
    HIPCHK(hipMemsetAsync(s->pl_score, 0, (size_t)K * sizeof(uint32_t), c->stream));
    for (int32_t k0 = 0; k0 < K; k0 += kPlaneChunk)
      hipLaunchKernelGGL(k_pl_score, grid, dim3(kVoxBlock), 0, c->stream, (const double*)s->cent.get(), d_among, M,
                         (const double*)s->pl_hyp.get(), k0, std::min<int32_t>(kPlaneChunk, K - k0), s->pl_score.get());
  }
  HIPCHK(hipGetLastError());
  // pick, on the host: the scores come back with the call's first synchronisation
  std::vector<uint32_t> score((size_t)K);
  if (int r = copy_back(c, score.data(), s->pl_score, score.size() * sizeof(uint32_t))) return r;
  const int32_t k = plane_pick(score.data(), K);
  if (k < 0) {   // no valid hypothesis with three inliers: an all-false mask and the zero model
    HIPCHK(hipMemsetAsync(s->pl_mask, 0, (size_t)M, c->stream));
    if (d_inliers) HIPCHK(hipMemsetAsync(d_inliers, 0, (size_t)M, c->stream));
    return MC_OK;
  }
  PlaneHyp h;
  static_assert(sizeof(PlaneHyp) == kPlaneHyp * sizeof(double), "the hypothesis record");
  HIPCHK(hipMemcpyAsync(&h, s->pl_hyp + (size_t)kPlaneHyp * k, sizeof h, hipMemcpyDeviceToHost, c->stream));
  if (int r = copy_back(c, samples, s->pl_samples + (size_t)3 * k, 3 * sizeof(int32_t))) return r;
  const double raw[4] = {h.n[0], h.n[1], h.n[2], h.d};
  int64_t n_in = 0;
  if (int r = plane_mask(c, s, d_among, raw, h.tau, false, &n_in)) return r;
  if (n_in != (int64_t)score[k])
    return fail(MC_ERR_STATE, "voxel plane: hypothesis %d scored %u and holds %lld voxels", k, score[k], (long long)n_in);
  stats[0] = k;
  stats[1] = (int64_t)score[k];
  if (refine) {
    double sums[kPlaneSums], C[6];
    if (int r = plane_moments(c, s, h.p0, sums)) return r;
    plane_refit(sums, (int32_t)n_in, h.p0, model, C);
    if (cov) std::copy_n(C, 6, cov);
    if (int r = plane_mask(c, s, d_among, model, distance, true, &n_in)) return r;
    stats[3] = 1;
  } else {
    plane_model(h, model);
  }
  stats[2] = n_in;
  if (d_inliers) HIPCHK(hipMemcpyAsync(d_inliers, s->pl_mask, (size_t)M, hipMemcpyDeviceToDevice, c->stream));
  return MC_OK;
}

int mc_voxel_emit_selected(mc_ctx* c, const uint8_t* d_mask, mc_batch* out) {
  CHECK_ARG(c && out, "NULL argument");
  CHECK_ARG(out->ctx == c, "batch belongs to another context");
  VoxState* s;
  if (int r = live_build(c, "mc_voxel_emit_selected", &s)) return r;
  CHECK_ARG(s->M == 0 || d_mask, "d_mask is NULL");
  DeviceGuard g(c->device);
  int64_t n = 0;
  if (s->M > 0) if (int r = compact(c, s, d_mask, kPlSelect, &n)) return r;
  CHECK_ARG(out->F == 1 && out->N == n, "the out batch must be one frame of exactly %lld points (it has %d frames, %lld points)",
            (long long)n, out->F, (long long)out->N);
  if (out->P > 0) {
    VoxOut a = out_of(s);
    a.cols = out->d_cols;
    a.C = out->C;
    {
      TimedRegion tr(c, &s->ev[kPlSelect], c->stream);
      hipLaunchKernelGGL(k_pl_emit_selected, dim3(blocks_of(out->P / 4)), dim3(kVoxBlock), 0, c->stream, a, out->P,
                         (const uint32_t*)s->pl_ids.get(), n);
    }
    HIPCHK(hipGetLastError());
  }
  return mcimpl::batch_columns_written(out, mcimpl::kWroteAllQueued);
}

int mc_timing_read_plane(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kPlanePhases, ms_phase, launches);
}

int mc_voxel_nearest_batch(mc_ctx* c, const mc_batch* src, int32_t frame, double max_distance, const double* transform,
                           int32_t* d_ids, double* d_dist2) {
  CHECK_ARG(c, "ctx is NULL");
  RegSrc s;
  if (int r = reg_source_batch(c, src, frame, &s)) return r;
  return nearest_run<true>(c, s, max_distance, transform, d_ids, d_dist2, "mc_voxel_nearest_batch");
}

int mc_voxel_nearest_f64(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, double max_distance, const double* transform,
                         int32_t* d_ids, double* d_dist2) {
  CHECK_ARG(c, "ctx is NULL");
  RegSrc s;
  if (int r = reg_source_rows(d_rows, ld, n, &s)) return r;
  return nearest_run<false>(c, s, max_distance, transform, d_ids, d_dist2, "mc_voxel_nearest_f64");
}

static void register_clear(double* transformation, int64_t* stats) {
  if (transformation) std::fill_n(transformation, 16, 0.0);
  if (stats) { stats[0] = stats[1] = stats[3] = 0; stats[2] = -1; }
}

int mc_voxel_register_batch(mc_ctx* c, const mc_batch* src, int32_t frame, const mc_register_params* p, double* transformation,
                            double* history, int64_t* stats) {
  register_clear(transformation, stats);
  CHECK_ARG(c && p && transformation && history && stats, "NULL argument");
  RegSrc s;
  if (int r = reg_source_batch(c, src, frame, &s)) return r;
  return register_run<true>(c, s, p, transformation, history, stats, "mc_voxel_register_batch");
}

int mc_voxel_register_f64(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, const mc_register_params* p,
                          double* transformation, double* history, int64_t* stats) {
  register_clear(transformation, stats);
  CHECK_ARG(c && p && transformation && history && stats, "NULL argument");
  RegSrc s;
  if (int r = reg_source_rows(d_rows, ld, n, &s)) return r;
  return register_run<false>(c, s, p, transformation, history, stats, "mc_voxel_register_f64");
}

int mc_voxel_register_frames(mc_ctx* c, const mc_batch* src, const mc_register_params* p, const double* inits,
                             double* transformations, double* history, int64_t* stats) {
  CHECK_ARG(c && src && p && transformations && history && stats, "NULL argument");
  CHECK_ARG(src->ctx == c, "batch belongs to another context");
  for (int32_t f = 0; f < src->F; ++f) register_clear(transformations + 16 * (size_t)f, stats + 4 * (size_t)f);
  return register_frames_run(c, src, p, inits, transformations, history, stats, "mc_voxel_register_frames");
}

int mc_timing_read_register_frames(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kRegFramesPhases, ms_phase, launches);
}

int mc_timing_read_register(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  if (int r = read_phases(c, kRegPhases, ms_phase, launches)) return r;
  // the solve's slot, by the host's clock
  VoxState* s = state_of(c, false);
  if (ms_phase) ms_phase[kRgSolve] = s ? s->rg_solve_ms : 0.0;
  if (s) {
    if (launches) *launches += s->rg_solve_n;
    s->rg_solve_ms = 0.0;
    s->rg_solve_n = 0;
  }
  return MC_OK;
}

static void rays_clear(int64_t* stats) {
  if (stats) std::fill_n(stats, 4, (int64_t)0);
}

int mc_voxel_rays_batch(mc_ctx* c, const mc_batch* src, int32_t frame, const double* origins, int64_t n_origins, int32_t guard,
                        int32_t max_steps, int32_t* d_passed, int32_t* d_ended, int32_t* d_through, int64_t* stats) {
  rays_clear(stats);
  CHECK_ARG(c && stats, "ctx or stats is NULL");
  RegSrc rs;   // the checks of a source, and its first point and their number
  if (int r = reg_source_batch(c, src, frame, &rs)) return r;
  CHECK_ARG(origins, "origins is NULL");
  CHECK_ARG(n_origins == 1 || n_origins == src->F, "origins must be 1 or %d (one per frame) rows of 3, got %lld", src->F,
            (long long)n_origins);
  for (int64_t k = 0; k < 3 * n_origins; ++k)
    CHECK_ARG(std::isfinite(origins[k]), "origins must be finite (row %lld, axis %d: %g)", (long long)(k / 3), (int)(k % 3), origins[k]);
  VoxState* s;
  if (int r = rays_checks(c, guard, max_steps, d_passed, d_ended, d_through, "mc_voxel_rays_batch", &s)) return r;
  DeviceGuard g(c->device);
  if (int r = ctx_reserve(c, s->ry_origins, (size_t)(3 * n_origins))) return r;
  HIPCHK(hipMemcpyAsync(s->ry_origins, origins, (size_t)(3 * n_origins) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  RaysArgs a = {};
  a.src = batch_source(src);
  a.slot0 = frame < 0 ? 0 : src->poff[frame];
  a.slots = frame < 0 ? src->P : src->poff[frame + 1] - src->poff[frame];
  a.first = rs.first;
  a.origins = s->ry_origins;
  a.n_origins = n_origins;
  return rays_run<true>(c, s, a, rs.n, a.slots, guard, max_steps, d_passed, d_ended, d_through, stats);
}

int mc_voxel_rays_f64(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, const double* d_origins, int64_t n_origins,
                      int32_t guard, int32_t max_steps, int32_t* d_passed, int32_t* d_ended, int32_t* d_through, int64_t* stats) {
  rays_clear(stats);
  CHECK_ARG(c && stats, "ctx or stats is NULL");
  RegSrc rs;
  if (int r = reg_source_rows(d_rows, ld, n, &rs)) return r;
  CHECK_ARG(d_origins, "d_origins is NULL");
  CHECK_ARG(n_origins == 1 || n_origins == n, "origins must be 1 or %lld (one per row) rows of 3, got %lld", (long long)n,
            (long long)n_origins);
  VoxState* s;
  if (int r = rays_checks(c, guard, max_steps, d_passed, d_ended, d_through, "mc_voxel_rays_f64", &s)) return r;
  DeviceGuard g(c->device);
  RaysArgs a = {};
  a.src.rows = d_rows; a.src.ld = ld; a.src.n = n;
  a.origins = d_origins;
  a.n_origins = n_origins;
  return rays_run<false>(c, s, a, n, n, guard, max_steps, d_passed, d_ended, d_through, stats);
}

int mc_timing_read_voxel_rays(mc_ctx* c, double* ms_phase, int64_t* launches) {
  CHECK_ARG(c, "ctx is NULL");
  return read_phases(c, kRaysPhases, ms_phase, launches);
}

int mc_voxel_release(mc_ctx* c) {
  if (!c) return MC_OK;
  VoxState* s = state_of(c, false);
  if (!s) return MC_OK;
  DeviceGuard g(c->device);
  (void)sync_all(c);
  for (auto& v : s->ev) ev_recycle(c, v);
  c->ext[mcimpl::kSlotVoxel].reset();
  return MC_OK;
}

}  // extern "C"
