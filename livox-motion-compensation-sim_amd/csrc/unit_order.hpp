// unit_order.hpp — the workgroup -> unit orders of the deskew, stager, scan and codec kernels (layout.hpp):
// xcd_unit and stream_unit, on plain integers.  A core header (DESIGN.md "Core headers"): the device compiles
// this text and so does tests/host/stream_order_host.cpp.  Needs no stand-in.  No HIP include.
#pragma once
#include <stdint.h>

#include "core_fn.hpp"

namespace mc {

// XCD-aware unit order.  Workgroups are dealt round-robin over the 8 XCDs (observed; speed only,
// never correctness): unit order b -> contiguous runs per XCD, so the 16-byte per-unit records
// (tiles, sub-tile windows) of neighbouring units share 128-byte lines inside one XCD's L2
// instead of each workgroup fetching its own line.  A bijection on [0, n) for any n.
constexpr int kXcds = 8;
template <bool ON>
MC_CORE_DEV int64_t xcd_unit(int64_t b, int64_t n) {
  if (!ON) return b;
  const int64_t x = b % kXcds, i = b / kXcds, per = n / kXcds, rem = n % kXcds;
  return x * per + (x < rem ? x : rem) + i;
}

// Stream order of a launch over n units (workgroup b -> unit): bit 1 = the 8 contiguous XCD ranges of
// xcd_unit<true> (else in order), bit 0 = reversed (within each range).  Codec kernels take the order
// that starts where the previous kernel over the same batch ended (mc_batch::hot_order), while those
// points may still sit in the 256 MB Infinity Cache.  A bijection on [0, n) for any n.
MC_CORE_DEV int64_t stream_unit(int order, int64_t b, int64_t n) {
  const bool rev = (order & 1) != 0;
  if (order & 2) {
    const int64_t x = b % kXcds, i = b / kXcds, per = n / kXcds, rem = n % kXcds;
    const int64_t len = per + (x < rem ? 1 : 0), start = x * per + (x < rem ? x : rem);
    return start + (rev ? len - 1 - i : i);
  }
  return rev ? n - 1 - b : b;
}

}  // namespace mc
