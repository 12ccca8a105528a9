// time_rule.hpp — the "evenly timed frame" rule of the per-point deskew kernels, on plain integers so
// the same text compiles for the device (kernels.hpp: k_trange tests it, k_deskew_points<.., RULE = true>
// generates from it) and for the host (tests/test_time_rule_cpu.py builds it with g++).  No HIP include.
//
// A frame with n valid points is evenly timed when its stored column is the ramp of its first two
// values,
//   t_ns[i] == time_rule_at(t0, dt, i)  for every valid i,   t0 = t_ns[0],  dt = t_ns[1] - t_ns[0]
// (dt = 0 when n < 2; n = 0 is evenly timed and never read).  Such a frame's time column need not be
// loaded: the kernel forms the same value from (t0, dt) and the point's index within its frame.
//
// ONE arithmetic decides both sides: int32 wrap-around (two's complement, i.e. uint32 modulo 2^32).
// dt is the wrapped difference, i * dt the wrapped product, the sum wraps.  The predicate compares the
// stored value with exactly what the kernel generates, so whatever it accepts — a ramp whose i * dt
// leaves int32 included: the stored column then has to hold the wrapped values — is reproduced to the
// bit.  Nothing else is promised: a column that is a ramp in int64 but leaves int32 could not have
// been stored in the int32 column in the first place.
#pragma once
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

// What the deskew kernel fetches per frame with one 16-byte scalar load: the frame's first padded
// point (local index = p - poff) and the ramp.  even != 0 only in mc_batch's host-side summary; the
// device record of a frame that is not evenly timed is never used to generate (a batch with one such
// frame keeps the loading kernel).
struct TimeRule {
  int64_t poff;
  int32_t t0, dt;
};
static_assert(sizeof(TimeRule) == 16, "one s_load_dwordx4");

// the step of a frame whose first two stored times are a, b
MC_CORE_HD int32_t time_rule_step(int32_t a, int32_t b) { return (int32_t)((uint32_t)b - (uint32_t)a); }

// the time the rule generates for frame-local index i (0 <= i < 2^32; only its low 32 bits matter)
MC_CORE_HD int32_t time_rule_at(int32_t t0, int32_t dt, int64_t i) {
  return (int32_t)((uint32_t)t0 + (uint32_t)(uint64_t)i * (uint32_t)dt);
}

// does the stored time t of frame-local index i follow the rule?
MC_CORE_HD bool time_rule_holds(int32_t t0, int32_t dt, int64_t i, int32_t t) {
  return time_rule_at(t0, dt, i) == t;
}

// host restatement over one frame's n valid stored times: 1 when evenly timed (t0, dt as defined above;
// both 0 for n = 0)
inline int time_rule_frame(const int32_t* t, int64_t n, int32_t* t0, int32_t* dt) {
  *t0 = n > 0 ? t[0] : 0;
  *dt = n > 1 ? time_rule_step(t[0], t[1]) : 0;
  for (int64_t i = 0; i < n; ++i)
    if (!time_rule_holds(*t0, *dt, i, t[i])) return 0;
  return 1;
}

}  // namespace mc
