// batch_state.hpp — the two pieces of host bookkeeping every deskew call depends on, as plain C++ with
// named transitions: what a batch's caches still describe (BatchState, a member of mc_batch) and how
// the step scheduler issues k_prep over the two table halves (PrepSchedule, a member of mc_ctx).  No
// HIP include: tests/test_batch_state_cpu.py builds tests/host/batch_state_host.cpp with g++ alone.
//
// The library touches neither type's fields: a routine says what happened (an event) or asks what
// holds (a query).  Which routine raises which event is DESIGN.md §4.1.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cstddef>
#include <vector>

namespace mcimpl {

// ------------------------------------------------------------------------------------------------
// What is cached about a batch's columns, and whether it still describes them.
//   sums   the ASCII PCD text bytes per block (MC_BATCH_WITH_PCD_LEN), written by some kernels
//          together with the x|y|z|intensity columns
//   intensity  whose intensity column this batch holds: a deskew passes the input's through unchanged, so
//          a later deskew of the same input into this batch need not move it while neither was written
//   spans per frame and per sub-tile [min, max] of t_ns, and with them the evenly-timed rule
//          (time_rule.hpp): one pass makes both, so the rule is valid exactly when the spans are
//   key    the version of everything k_prep reads from the batch: frame times, frame starts, spans
//   rel    mc_deskew_relative's table: its offsets hold for a (trajectory, key), its records for
//          that and one set of reference times
// ------------------------------------------------------------------------------------------------
class BatchState {
 public:
  // ---- events ----
  // a write of the point columns (x|y|z|intensity) is about to be queued: whatever sums exist are stale
  void points_written() { ++data_ver_; }
  // the write announced last also wrote the sums (the caller knows the batch has a sums buffer)
  void sums_written() { sums_ver_ = data_ver_; }
  // the write announced last left this batch's intensity column equal to that of the batch `src_uid`
  // at its points version `src_ver` (a deskew out of that batch: the column is passed through)
  void intensity_copied_from(uint64_t src_uid, uint64_t src_ver) {
    int_uid_ = src_uid;
    int_src_ver_ = src_ver;
    int_own_ver_ = data_ver_;
  }
  // the t_ns column was written: spans and rule describe another column until spans_computed().  The
  // key moves there, not here: every reader of the spans (the per-point modes' k_prep, the relative
  // table) recomputes them first, and frame mode's prep does not read them.
  void time_written() { spans_valid_ = false; }
  // the span pass ran over the present column; even: every non-empty frame is on its ramp
  void spans_computed(bool even) {
    spans_valid_ = true;
    time_even_ = even;
    ++prep_ver_;
  }
  // a batch without frames or without a time column has no spans to make: current, and no rule
  void spans_not_needed() { spans_valid_ = true; }
  void frame_times_set() { has_times_ = true; ++prep_ver_; }
  void frame_starts_set() { has_starts_ = true; ++prep_ver_; }
  // the relative table is about to be rebuilt (its records always, its offsets too if asked): a
  // failure on the way leaves nothing reusable
  void rel_rebuilding(bool offsets_too) {
    rel_valid_ = false;
    if (offsets_too) rel_offsets_valid_ = false;
  }
  // ... its offsets were counted for trajectory upload `traj` and the present key
  void rel_offsets_built(uint64_t traj) {
    rel_traj_ = traj;
    rel_frames_ = prep_ver_;
    rel_offsets_valid_ = true;
  }
  // ... its records were composed for the F reference times t_ref (null: each frame's own time)
  void rel_built(const double* t_ref, size_t F) {
    rel_own_ = t_ref == nullptr;
    if (t_ref) rel_tref_.assign(t_ref, t_ref + F); else rel_tref_.clear();
    rel_valid_ = true;
  }

  // ---- queries ----
  bool sums_current() const { return sums_ver_ == data_ver_; }
  uint64_t points_version() const { return data_ver_; }   // what a holder of this batch's intensity records
  // does this batch hold the intensity of batch `src_uid` as of its points version `src_ver`?  Neither
  // batch's point columns were written since the copy (uid 0 is no batch: nothing copied yet)
  bool holds_intensity_of(uint64_t src_uid, uint64_t src_ver) const {
    return int_uid_ != 0 && int_uid_ == src_uid && int_src_ver_ == src_ver && int_own_ver_ == data_ver_;
  }
  bool spans_current() const { return spans_valid_; }
  bool rule_usable() const { return spans_valid_ && time_even_; }
  bool has_frame_times() const { return has_times_; }
  bool has_frame_starts() const { return has_starts_; }
  uint64_t prep_key() const { return prep_ver_; }   // the batch's component of a PrepKey
  bool rel_offsets_reusable(uint64_t traj) const {
    return rel_offsets_valid_ && rel_traj_ == traj && rel_frames_ == prep_ver_;
  }
  bool rel_reusable(uint64_t traj, const double* t_ref, size_t F) const {
    const bool same_ref = rel_own_ == (t_ref == nullptr) &&
                          (!t_ref || (rel_tref_.size() == F && std::equal(t_ref, t_ref + F, rel_tref_.begin())));
    return rel_offsets_reusable(traj) && rel_valid_ && same_ref;
  }

 private:
  // data_ver_ counts the writes of the point columns; sums_ver_ is the one the sums came with
  uint64_t data_ver_ = 1, sums_ver_ = 0;
  // whose intensity the column holds: the source's uid and points version, and data_ver_ as of the copy
  uint64_t int_uid_ = 0, int_src_ver_ = 0, int_own_ver_ = 0;
  uint64_t prep_ver_ = 0;
  bool spans_valid_ = false, time_even_ = false;
  bool has_times_ = false, has_starts_ = false;
  bool rel_offsets_valid_ = false, rel_valid_ = false, rel_own_ = false;
  uint64_t rel_traj_ = 0, rel_frames_ = 0;
  std::vector<double> rel_tref_;
};

// Everything a step's k_prep reads, by version: the input batch (its uid: a key never matches a new
// batch; its BatchState::prep_key), the trajectory and IMU uploads, mode and pose selection.
struct PrepKey {
  uint64_t batch = 0, traj = 0, imu = 0, frames = 0;   // batch 0: no call
  int mode = -1, pose_select = -1;
  bool operator==(const PrepKey& o) const {
    return batch == o.batch && traj == o.traj && imu == o.imu && frames == o.frames && mode == o.mode &&
           pose_select == o.pose_select;
  }
};

// ------------------------------------------------------------------------------------------------
// How k_prep is issued.  One queue (the context's main stream) and two halves of every per-step
// table: a step's prep writes the free half while the previous step's deskew kernel may still read
// the other; the deskew kernel two steps back read the free half and has finished, because its
// successor's packet waited for it.
//
// The contract of an any-order prep (a packet with the barrier bit clear, which may start before the
// packets ahead of it finish).  It is allowed only right behind this context's own plain deskew
// kernel — the fence is clear: the packets before it are then that kernel, still reading the other
// half, and, before it, work the kernel's barrier already waited for.  Everything else that could
// precede it either finished before its API call returned (trajectory, IMU and frame tables are
// uploaded synchronously) or set the fence with work_in_flight(): the t_ns span pass, the stagers,
// the decoders and the voxel emit, an affine transform, a speculative launch, whose prep workgroups
// write the very half the next prep would.  The deskew kernel's own packet keeps the barrier bit, so
// it waits for its prep, and anything queued after it waits for both.  With no kernel to follow (no
// tiles) the prep is ordinary and the fence stays set.
//
// Speculation.  A call whose key equals the previous call's launches its deskew fused with the prep
// of an identical next call into the other half; that next call, if its key still matches and it got
// that half, finds its tables ready (a hit) and issues no k_prep.  Whatever writes a half outside
// this bookkeeping forgets the speculation first.
// ------------------------------------------------------------------------------------------------
class PrepSchedule {
 public:
  struct Decision {
    bool prep;        // issue k_prep (false: a hit)
    bool any_order;   // ... as an any-order packet
    bool speculate;   // launch the deskew fused with the next identical call's prep into half h ^ 1
  };

  // the half the next prep may write: the one the last deskew kernel does not read
  int free_half() const { return buf_; }
  // ... is taken by the caller's step (what it returns), and the other becomes free
  int take_half() {
    const int h = buf_;
    buf_ ^= 1;
    return h;
  }
  // the caller leaves work queued that a prep must not overtake
  void work_in_flight() { fence_ = true; }
  // a table half is written outside the key bookkeeping: no speculated tables stay valid, and the
  // next call does not speculate from a key seen before
  void forget_speculation() {
    spec_valid_ = false;
    last_call_ = PrepKey{};
  }
  // One mc_deskew with this key, writing half h (taken just before); kernel: a deskew launch follows
  // (the batch has tiles); may_fuse: that launch has a fused next-prep variant (not the PCD kernels,
  // which may still hit).  Followed by launched_speculative() or launched_plain() when kernel.
  Decision decide(const PrepKey& key, int h, bool kernel, bool may_fuse) {
    const bool hit = spec_valid_ && spec_half_ == h && spec_key_ == key;
    const Decision d{!hit, !hit && !fence_ && kernel, kernel && may_fuse && last_call_ == key};
    last_call_ = key;
    spec_valid_ = false;
    if (!kernel) fence_ = true;
    return d;
  }
  // the fused launch decide() asked for was issued: half h ^ 1 holds the tables of `key`, and the next
  // prep (on a miss) would write the half these prep workgroups write
  void launched_speculative(const PrepKey& key, int h) {
    spec_valid_ = true;
    spec_half_ = h ^ 1;
    spec_key_ = key;
    fence_ = true;
  }
  // a plain deskew kernel ends the queue: the next prep may run beside it
  void launched_plain() { fence_ = false; }
  // may the first prep of a run of pipelined steps be any-order?
  bool prep_may_overtake() const { return !fence_; }
  // n pipelined steps were issued, step i reading half h0 ^ (i & 1) (each launch but the last fused
  // with the next step's prep, the last one plain): the free half is the one the last did not read
  void steps_issued(int h0, int n) {
    forget_speculation();
    buf_ = h0 ^ (n & 1);
    fence_ = false;
  }
  // the tuner's launches may have read and written either half
  void tuner_ran() {
    forget_speculation();
    fence_ = true;
  }

 private:
  int buf_ = 0;
  bool fence_ = true;     // the next k_prep waits for everything queued before it
  PrepKey last_call_;     // the previous mc_deskew's key
  PrepKey spec_key_;      // what the tables in half spec_half_ were prepared for
  bool spec_valid_ = false;
  int spec_half_ = 0;
};

}  // namespace mcimpl
