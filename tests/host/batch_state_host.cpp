// Host driver of csrc/batch_state.hpp for tests/test_batch_state_cpu.py: scripted event sequences
// through the two state machines, each decision checked against the rules written in the header (not
// against a run of the library).  Prints "ok <scenario>" per scenario; the first failed check ends the
// program with its line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "batch_state.hpp"

using mcimpl::BatchState;
using mcimpl::PrepKey;
using mcimpl::PrepSchedule;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

namespace {
struct Call {
  PrepSchedule::Decision d;
  int h;
};
// one mc_deskew as the library drives the schedule: take the free half, decide, report the launch
Call call(PrepSchedule& s, const PrepKey& k, bool kernel = true, bool may_fuse = true) {
  const int h = s.take_half();
  const PrepSchedule::Decision d = s.decide(k, h, kernel, may_fuse);
  if (kernel) {
    if (d.speculate) s.launched_speculative(k, h);
    else s.launched_plain();
  }
  return {d, h};
}
bool is(const PrepSchedule::Decision& d, bool prep, bool any_order, bool speculate) {
  return d.prep == prep && d.any_order == any_order && d.speculate == speculate;
}
const PrepKey kKey{7, 1, 1, 3, 1, 0};

// a schedule after three identical calls: the third was a hit on the tables the second speculated
PrepSchedule after_hit(int* last_half) {
  PrepSchedule s;
  call(s, kKey);
  call(s, kKey);
  const Call c = call(s, kKey);
  CHECK(!c.d.prep);
  *last_half = c.h;
  return s;
}

void three_identical_calls() {
  PrepSchedule s;
  int preps = 0;
  // a fresh context starts fenced (batch creation, uploads): an ordinary prep, nothing to speculate from
  Call c = call(s, kKey);
  CHECK(is(c.d, true, false, false) && c.h == 0);
  preps += c.d.prep;
  // the same key again, right behind a plain kernel: any-order, and its launch prepares the third call
  c = call(s, kKey);
  CHECK(is(c.d, true, true, true) && c.h == 1);
  preps += c.d.prep;
  // a hit: no prep at all; it speculates for the fourth
  c = call(s, kKey);
  CHECK(is(c.d, false, false, true) && c.h == 0);
  preps += c.d.prep;
  CHECK(preps == 2);
  c = call(s, kKey);
  CHECK(is(c.d, false, false, true) && c.h == 1);
}

void key_change_misses() {
  for (int comp = 0; comp < 6; ++comp) {
    int h_prev = -1;
    PrepSchedule s = after_hit(&h_prev);
    PrepKey k = kKey;
    if (comp == 0) k.batch += 1;
    if (comp == 1) k.traj += 1;
    if (comp == 2) k.imu += 1;
    if (comp == 3) k.frames += 1;
    if (comp == 4) k.mode = 2;
    if (comp == 5) k.pose_select = 1;
    // a miss: a prep, ordinary (the hit's launch was speculative: its prep workgroups wrote this very
    // half), nothing to speculate from; into the half the previous kernel does not read
    const Call c = call(s, k);
    CHECK(is(c.d, true, false, false));
    CHECK(c.h == (h_prev ^ 1));
    // the new key a second time: behind a plain kernel, and now it repeats
    CHECK(is(call(s, k).d, true, true, true));
    CHECK(is(call(s, k).d, false, false, true));
  }
}

void work_in_flight_fences() {
  // between two plain calls
  PrepSchedule s;
  call(s, kKey);
  s.work_in_flight();
  CHECK(is(call(s, kKey).d, true, false, true));
  // between a miss behind a plain kernel and the next: the same
  PrepSchedule t;
  PrepKey other = kKey;
  other.batch = 8;
  call(t, kKey);
  CHECK(is(call(t, other).d, true, true, false));
  t.work_in_flight();
  CHECK(is(call(t, kKey).d, true, false, false));
  // a hit needs no prep, whatever was queued since
  int h = -1;
  PrepSchedule u = after_hit(&h);
  u.work_in_flight();
  CHECK(is(call(u, kKey).d, false, false, true));
}

void fence_after_each_launch() {
  PrepKey other = kKey;
  other.mode = 0;
  // after a plain launch the next prep may be any-order
  PrepSchedule s;
  CHECK(is(call(s, kKey).d, true, false, false));
  CHECK(is(call(s, other).d, true, true, false));
  // after a speculative launch the next prep (on a miss) is ordinary
  PrepSchedule t;
  call(t, kKey);
  CHECK(call(t, kKey).d.speculate);
  CHECK(is(call(t, other).d, true, false, false));
  // a launch with no fused variant (the PCD kernels) never speculates, but it may hit
  PrepSchedule u;
  call(u, kKey);
  CHECK(call(u, kKey).d.speculate);
  CHECK(is(call(u, kKey, true, false).d, false, false, false));
  CHECK(is(call(u, kKey, true, false).d, true, true, false));
}

void no_kernel() {
  // no tiles: an ordinary prep, and the fence stays set — also when it was clear before
  PrepSchedule s;
  CHECK(is(call(s, kKey, false).d, true, false, false));
  CHECK(!s.prep_may_overtake());
  CHECK(is(call(s, kKey, false).d, true, false, false));
  PrepSchedule t;
  call(t, kKey);
  CHECK(t.prep_may_overtake());
  CHECK(is(call(t, kKey, false).d, true, false, false));
  CHECK(!t.prep_may_overtake());
  CHECK(is(call(t, kKey).d, true, false, true));
}

void pipelined_steps() {
  for (int n = 1; n <= 3; ++n)
    for (int flip = 0; flip < 2; ++flip) {
      PrepSchedule s;
      if (flip) s.take_half();
      call(s, kKey);
      CHECK(call(s, kKey).d.speculate);   // tables of kKey wait in the other half
      s.forget_speculation();
      const int h0 = s.free_half();
      s.steps_issued(h0, n);
      CHECK(s.free_half() == (h0 ^ (n & 1)));
      CHECK(s.prep_may_overtake());
      // speculation forgotten: no hit, and nothing to speculate from; the fence is clear
      CHECK(is(call(s, kKey).d, true, true, false));
    }
}

void tuner() {
  PrepSchedule s;
  call(s, kKey);
  CHECK(call(s, kKey).d.speculate);
  s.tuner_ran();
  CHECK(!s.prep_may_overtake());
  CHECK(is(call(s, kKey).d, true, false, false));
}

void forget_speculation() {
  // a transform takes a half and writes it: the tables speculated for the next call are gone
  PrepSchedule s;
  call(s, kKey);
  CHECK(call(s, kKey).d.speculate);
  const int h = s.take_half();
  CHECK(h == 0);
  s.forget_speculation();
  s.work_in_flight();
  CHECK(is(call(s, kKey).d, true, false, false));
}

void batch_sums() {
  BatchState b;
  CHECK(!b.sums_current());
  b.points_written();
  CHECK(!b.sums_current());
  b.points_written();
  b.sums_written();
  CHECK(b.sums_current());
  b.time_written();   // another column: the sums stay
  CHECK(b.sums_current());
  b.points_written();
  CHECK(!b.sums_current());
}

void batch_spans_and_key() {
  BatchState b;
  CHECK(!b.spans_current() && !b.rule_usable());
  CHECK(!b.has_frame_times() && !b.has_frame_starts());
  uint64_t k = b.prep_key();
  b.spans_computed(true);
  CHECK(b.spans_current() && b.rule_usable() && b.prep_key() != k);
  k = b.prep_key();
  b.points_written();   // the point columns are not the time column
  CHECK(b.spans_current() && b.rule_usable() && b.prep_key() == k);
  b.time_written();
  CHECK(!b.spans_current() && !b.rule_usable());
  b.spans_computed(false);   // what every reader of the spans does first
  CHECK(b.spans_current() && !b.rule_usable() && b.prep_key() != k);
  k = b.prep_key();
  b.time_written();
  b.spans_computed(true);
  CHECK(b.rule_usable() && b.prep_key() != k);
  k = b.prep_key();
  b.frame_times_set();
  CHECK(b.has_frame_times() && !b.has_frame_starts() && b.prep_key() != k);
  k = b.prep_key();
  b.frame_starts_set();
  CHECK(b.has_frame_starts() && b.prep_key() != k);
  CHECK(b.rule_usable());
  // no frames or no time column: nothing to compute, nothing changes for k_prep, and no rule
  BatchState e;
  k = e.prep_key();
  e.spans_not_needed();
  CHECK(e.spans_current() && !e.rule_usable() && e.prep_key() == k);
}

void batch_relative_table() {
  const double ref[2] = {1.5, 2.5}, ref2[2] = {1.5, 2.75};
  BatchState b;
  b.frame_times_set();
  b.spans_computed(false);
  CHECK(!b.rel_offsets_reusable(3) && !b.rel_reusable(3, nullptr, 2));
  b.rel_rebuilding(true);
  b.rel_offsets_built(3);
  CHECK(b.rel_offsets_reusable(3) && !b.rel_reusable(3, nullptr, 2));   // offsets only: a failed compose
  b.rel_built(nullptr, 2);
  CHECK(b.rel_reusable(3, nullptr, 2));
  CHECK(!b.rel_reusable(3, ref, 2));                                  // another reference
  CHECK(!b.rel_reusable(4, nullptr, 2) && !b.rel_offsets_reusable(4));   // another trajectory upload
  // explicit references: by value
  b.rel_rebuilding(false);
  CHECK(b.rel_offsets_reusable(3) && !b.rel_reusable(3, nullptr, 2));
  b.rel_built(ref, 2);
  const double same[2] = {1.5, 2.5};
  CHECK(b.rel_reusable(3, same, 2));
  CHECK(!b.rel_reusable(3, ref2, 2) && !b.rel_reusable(3, nullptr, 2) && !b.rel_reusable(3, same, 1));
  // the key component moves (here: new spans): neither part survives, and a rebuild restores both
  b.time_written();
  b.spans_computed(false);
  CHECK(!b.rel_offsets_reusable(3) && !b.rel_reusable(3, same, 2));
  b.rel_rebuilding(true);
  b.rel_offsets_built(3);
  b.rel_built(same, 2);
  CHECK(b.rel_reusable(3, ref, 2));
  b.frame_times_set();
  CHECK(!b.rel_offsets_reusable(3) && !b.rel_reusable(3, ref, 2));
}

const struct {
  const char* name;
  void (*run)();
} kScenarios[] = {
    {"three_identical_calls", three_identical_calls},
    {"key_change_misses", key_change_misses},
    {"work_in_flight_fences", work_in_flight_fences},
    {"fence_after_each_launch", fence_after_each_launch},
    {"no_kernel", no_kernel},
    {"pipelined_steps", pipelined_steps},
    {"tuner", tuner},
    {"forget_speculation", forget_speculation},
    {"batch_sums", batch_sums},
    {"batch_spans_and_key", batch_spans_and_key},
    {"batch_relative_table", batch_relative_table},
};
}  // namespace

int main() {
  for (const auto& s : kScenarios) {
    s.run();
    std::printf("ok %s\n", s.name);
    std::fflush(stdout);
  }
  return 0;
}
