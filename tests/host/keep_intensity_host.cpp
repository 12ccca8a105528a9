// Host driver of the intensity provenance in csrc/batch_state.hpp for tests/test_keep_intensity_cpu.py:
// scripted sequences of the events a deskew and the other writers of a batch raise, each answer of
// holds_intensity_of checked against the rule written in the header (not against a run of the library).
// Prints "ok <scenario>" per scenario; the first failed check ends the program with its line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "batch_state.hpp"

using mcimpl::BatchState;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

namespace {
struct Batch {
  uint64_t uid;
  BatchState state;
};
bool holds(const Batch& out, const Batch& in) {
  return out.state.holds_intensity_of(in.uid, in.state.points_version());
}
// What the library decides and reports for one deskew of in into out, in its order: the question
// first, then the write of out's point columns, then (the launch queued) the provenance.  Returns
// whether the launch could leave the intensity column alone.
bool deskew(const Batch& in, Batch& out, bool queued = true) {
  const bool keep = &in == &out || holds(out, in);
  out.state.points_written();
  if (queued && &in != &out) out.state.intensity_copied_from(in.uid, in.state.points_version());
  return keep;
}

void held_after_the_event() {
  Batch in{11}, out{12};
  CHECK(!holds(out, in));   // nothing copied yet
  CHECK(!holds(in, out));
  CHECK(!deskew(in, out));
  CHECK(holds(out, in));
  CHECK(!holds(in, out));   // the relation has a direction
  CHECK(!holds(out, out));
}

void own_write_then_event_holds_again() {
  Batch in{11}, out{12};
  CHECK(!deskew(in, out));
  for (int i = 0; i < 4; ++i) {
    CHECK(deskew(in, out));   // asked before the deskew's own points_written
    CHECK(holds(out, in));
  }
  // between the write and the event nothing is held: a launch that failed to queue claims nothing
  CHECK(deskew(in, out, false));
  CHECK(!holds(out, in));
  CHECK(!deskew(in, out));
  CHECK(holds(out, in));
}

void output_written() {
  Batch in{11}, out{12};
  deskew(in, out);
  out.state.points_written();   // an upload, an affine transform, a decoder into out
  CHECK(!holds(out, in));
  CHECK(!deskew(in, out));
  CHECK(holds(out, in));
  // events that leave the point columns alone leave the answer alone
  out.state.time_written();
  out.state.spans_computed(true);
  out.state.sums_written();
  in.state.frame_times_set();
  in.state.time_written();
  CHECK(holds(out, in));
}

void input_written() {
  Batch in{11}, out{12};
  deskew(in, out);
  in.state.points_written();   // synth with another seed, a stager into in
  CHECK(!holds(out, in));
  CHECK(!deskew(in, out));
  CHECK(holds(out, in));
}

void another_uid() {
  Batch a{11}, b{13}, out{12};
  deskew(a, out);
  CHECK(holds(out, a) && !holds(out, b));   // b at the same points version as a
  CHECK(a.state.points_version() == b.state.points_version());
  // a deskew of b into out replaces a's column
  CHECK(!deskew(b, out));
  CHECK(holds(out, b) && !holds(out, a));
  CHECK(!deskew(a, out));
  CHECK(holds(out, a) && !holds(out, b));
  // a new batch of the same shape has a new uid and a fresh state: it neither holds nor is held
  Batch out2{14}, a2{15};
  CHECK(!holds(out2, a) && !holds(out, a2));
  // uid 0 is no batch: a fresh state holds nothing of it either
  Batch none{0};
  CHECK(!holds(out2, none));
}

void stale_source_version() {
  Batch in{11}, out{12}, other{13};
  deskew(in, out);
  const uint64_t v = in.state.points_version();
  // in deskewed into another output, then written: out holds the column of a version that is gone
  deskew(in, other);
  CHECK(holds(out, in) && holds(other, in));
  in.state.points_written();
  CHECK(in.state.points_version() != v);
  CHECK(!holds(out, in) && !holds(other, in));
  CHECK(out.state.holds_intensity_of(in.uid, v));   // the record itself is untouched: only the source moved
  // in deskewed in place: its columns were written
  Batch in2{21}, out2{22};
  deskew(in2, out2);
  CHECK(deskew(in2, in2));
  CHECK(!holds(out2, in2));
}

void in_place_needs_no_state() {
  Batch b{11};
  CHECK(deskew(b, b));   // from the first call
  CHECK(!holds(b, b));   // and nothing is recorded
  CHECK(deskew(b, b));
}

void many_versions() {
  // the answer follows the versions however far they have moved, on either side
  Batch in{11}, out{12};
  for (int i = 0; i < 1000; ++i) {
    if (i % 3 == 0) in.state.points_written();
    if (i % 5 == 0) out.state.points_written();
    const bool fresh = i % 3 == 0 || i % 5 == 0 || i == 0;
    CHECK(deskew(in, out) == !fresh);
    CHECK(holds(out, in));
  }
}
}  // namespace

int main() {
#define RUN(f) f(), std::printf("ok %s\n", #f)
  RUN(held_after_the_event);
  RUN(own_write_then_event_holds_again);
  RUN(output_written);
  RUN(input_written);
  RUN(another_uid);
  RUN(stale_source_version);
  RUN(in_place_needs_no_state);
  RUN(many_versions);
  return 0;
}
