// internal.hpp — the opaque handles of include/mcdeskew.h, shared by every translation unit of the
// library: mcdeskew.hip (the context, the batches, the deskew paths and the host side of the two
// scanners), comm.cpp, codecs.hip and voxel.hip.  What only one feature reads — the scanners' and the
// codecs' state, and in the voxel slot the filter's with that of the analyses of its cloud (normals,
// clusters, planes and selection, registration) — is not here: it sits in that feature's slot of the context.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "batch_state.hpp"
#include "devbuf.hpp"

namespace mc {
struct Tile;
struct PoseSeg;
struct FrameRow;
struct ImuSeg;
struct FrameWin;
struct TimeRule;
}  // namespace mc

namespace mcimpl {
int fail(int code, const char* fmt, ...);
constexpr int64_t kBatchBlock = 256;   // points per block of the blocked batch layout (= mc::kBlkPts)

// Persistent host worker pool for the host-side row copies of the host<->device pipeline.
class HostPool {
 public:
  explicit HostPool(int threads) {
    for (int k = 0; k < threads; ++k) th_.emplace_back([this] { work(); });
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> l(m_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // fn(i) for i in [0, n) on the pool's threads; returns when all are done
  void run(int64_t n, const std::function<void(int64_t)>& fn) {
    if (n <= 0) return;
    std::unique_lock<std::mutex> l(m_);
    fn_ = &fn; n_ = n; next_ = 0; busy_ = (int)th_.size(); ++gen_;
    cv_.notify_all();
    done_.wait(l, [this] { return busy_ == 0; });
    fn_ = nullptr;
  }

 private:
  void work() {
    uint64_t seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> l(m_);
      cv_.wait(l, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      const std::function<void(int64_t)>* fn = fn_;
      const int64_t n = n_;
      l.unlock();
      for (int64_t i = next_++; i < n; i = next_++) (*fn)(i);
      l.lock();
      if (--busy_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int64_t)>* fn_ = nullptr;
  int64_t n_ = 0;
  std::atomic<int64_t> next_{0};
  int busy_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// What a context owns that is not memory.  A base of mc_ctx, so it is destroyed after every member:
// the buffers go first, then the pooled events, then the two streams.
struct CtxQueues {
  hipStream_t stream = nullptr;   // main stream: staging, k_prep and the deskew kernels (one queue)
  hipStream_t row_d2h = nullptr;  // the row pipeline's D2H copies, beside its H2D + kernel on `stream`
  std::vector<hipEvent_t> ev_pool;
  CtxQueues() = default;
  CtxQueues(const CtxQueues&) = delete;
  CtxQueues& operator=(const CtxQueues&) = delete;
  ~CtxQueues() {
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (row_d2h) (void)hipStreamDestroy(row_d2h);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
using EventPairs = std::vector<std::pair<hipEvent_t, hipEvent_t>>;

// State a feature's translation unit keeps in a context, one slot each (hostutil.hpp ctx_ext): only that
// unit defines the type.  Destroyed with the context's buffers, before the event pool and the streams.
struct CtxExt { virtual ~CtxExt() = default; };
enum CtxSlot { kSlotVoxel, kSlotScan, kSlotRay, kSlotCodec, kCtxSlots };
}  // namespace mcimpl
using mcimpl::DevBuf;
using mcimpl::EventPairs;

struct mc_ctx : mcimpl::CtxQueues {
  ~mc_ctx();   // mcdeskew.hip, where the records the buffers hold are complete types
  int device = 0;
  // which table half the next k_prep writes, whether it may be an any-order packet, and the per-call
  // speculation of mc_deskew: batch_state.hpp
  mcimpl::PrepSchedule sched;
  uint64_t traj_ver = 0, imu_ver = 0;   // bumped by mc_set_trajectory / mc_set_imu
  // sub-tile order per mode measured by mc_tune_order for batches of P padded points (-1: none)
  struct OrderTune {
    int64_t P = -1;
    int32_t order = -1;
  };
  OrderTune order_tune[3];
  // trajectory (LMC:361-428): time, position_gps, orientation_imu; host copies for the float64
  // paths' per-frame poses (rot.cpp frame_poses)
  int64_t T = 0, T_cap = 0;
  std::vector<double> h_time, h_pos, h_rpy;
  DevBuf<double> d_time;
  DevBuf<double> d_pos;
  DevBuf<double> d_rpy;
  DevBuf<mc::PoseSeg> d_pose_seg;      // 2 * T_cap (double buffer)
  // IMU (CSIM:1191-1240)
  int64_t M = 0, M_cap = 0;
  DevBuf<int64_t> d_imu_ts;
  DevBuf<double> d_gyro;
  DevBuf<mc::ImuSeg> d_imu_seg;        // 2 * M_cap (double buffer)
  // segment table of the float64 per-point path (mc_deskew_points_f64): built by k_prep for one mode
  // and the trajectory / IMU upload it came from (seg64_ver), rebuilt when either changes
  DevBuf<char> d_seg64;
  int seg64_mode = -1;
  uint64_t seg64_ver = 0;
  // pinned, device-mapped host buffer of the single-call drop-in path
  mcimpl::PinBuf<char, hipHostMallocMapped | hipHostMallocCoherent> h_pin;
  // host <-> device row pipeline (double-buffered pinned and device chunks, in + out)
  mcimpl::PinBuf<char, hipHostMallocDefault> h_pipe;
  DevBuf<char> d_pipe;
  std::unique_ptr<mcimpl::HostPool> pool;
  // staging buffer for host<->device layout conversion
  DevBuf<char> d_stage;
  // launch knobs / timing
  int32_t max_grid = 0;
  // evenly timed input batches take the deskew kernels that generate t_ns (mc_set_time_rule;
  // MCDESKEW_TIME_RULE=0 starts a context with it off)
  bool time_rule = true;
  // a per-point deskew into a batch that already holds the input's intensity column takes the kernels
  // that do not move it (mc_set_keep_intensity; MCDESKEW_KEEP_INTENSITY=0 starts a context with it off)
  bool keep_intensity = true;
  bool timing = false;
  double wall_khz = 0.0;   // wall_clock64() rate
  // workgroup spans of timed deskew launches (DeskewArgs::span): kSpanSlots slots of 1 + kSpanTail
  // wall-clock stamps, zeroed, handed out in launch order until mc_timing_read_spans
  DevBuf<unsigned long long> d_span;
  int32_t span_used = 0;
  EventPairs main_ev, prep_ev, layout_ev;
  // the features' own state, made on demand by their units (the voxel filter's is freed early by
  // mc_voxel_release).  The last member: destroyed first.
  std::unique_ptr<mcimpl::CtxExt> ext[mcimpl::kCtxSlots];
};

struct mc_batch {
  mc_ctx* ctx = nullptr;
  uint64_t uid = 0;         // unique per batch ever created (a key can never match a new batch)
  // what the caches below still describe (batch_state.hpp); mutable as they are: they belong to the
  // batch a deskew call reads
  mutable mcimpl::BatchState state;
  int32_t F = 0;
  int64_t N = 0;    // valid points
  int64_t P = 0;    // padded points (poff[F]; every frame starts on a kBlkPts boundary)
  int32_t C = 4;    // columns per block: x | y | z | intensity [| t_ns]
  std::vector<int64_t> counts, poff, doff;
  std::vector<int32_t> ftile;      // first tile of each frame (F+1), host copy
  int32_t n_tiles = 0;
  // stream_unit order (layout.hpp) of the last kernel that went over the batch's points: its last
  // units may still be in the Infinity Cache, so the codec kernels run the opposite direction
  // (a hint for speed only; kernels that do not record it leave it stale)
  mutable int hot_order = 0;
  // blocked columns: block k (points 256k .. 256k+255) holds its C columns of 256 values back to
  // back, C * P values in all (mc::bidx); t_ns, when present, is column 4 (int32 bits)
  DevBuf<float> d_cols;
  bool has_t() const { return C == 5; }
  DevBuf<int64_t> d_counts;
  DevBuf<int64_t> d_poff;
  DevBuf<int64_t> d_doff;
  DevBuf<mc::Tile> d_tiles;
  DevBuf<double> d_frame_time;
  DevBuf<int64_t> d_frame_start;
  // k_prep outputs, double-buffered (ctx->sched names the half): F entries per half
  DevBuf<mc::FrameRow> d_frame_tbl;   // 3 float64 rows per frame (R row, t)
  DevBuf<int2> d_trange;             // per-frame [min, max] t_ns (valid while state.spans_current())
  // the evenly-timed rule (time_rule.hpp), written by the same pass and valid exactly when the spans
  // are: per frame its ramp, and whether every valid point is on it ([F]: some frame of the batch is not)
  DevBuf<mc::TimeRule> d_trule;
  DevBuf<int32_t> d_teven;           // F + 1
  DevBuf<mc::FrameWin> d_fwin;       // per-frame segment window
  DevBuf<char> d_frec;               // 2 frame-specialised pose/IMU records per frame
  size_t frec_half = 0;              // bytes per half of d_frec
  // per sub-tile windows (batches with t_ns): frames wider than the SGPR path use these
  DevBuf<int32_t> d_ftile;            // first tile of each frame (F+1)
  DevBuf<int2> d_strange;            // per sub-tile [min, max] t_ns
  DevBuf<mc::FrameWin> d_swin;       // per sub-tile window, double-buffered (2 * n_sub)
  DevBuf<double> d_partial;
  // mc_deskew_relative: the per-frame relative segment table (relative.hpp) — frame f's records
  // [d_roff[f], d_roff[f+1]) are its segments [klo, khi] folded into its reference pose.  A cache kept
  // with the input batch, as its k_prep outputs are; state says what of it can be reused.
  mutable DevBuf<mc::PoseSeg> d_rel;
  mutable int64_t rel_total = 0;           // records in use (d_roff[F])
  mutable DevBuf<int64_t> d_roff;          // F + 1
  mutable DevBuf<int32_t> d_relw;          // F window widths (the count pass)
  mutable DevBuf<double> d_tref;           // F reference times
  mutable DevBuf<double> d_refpose;        // F reference quaternions (4 F), then F reference positions (3 F)
  // MC_BATCH_WITH_PCD_LEN: ASCII PCD text bytes per 256-point block (layout.hpp PcdCount sums),
  // current while state.sums_current()
  DevBuf<int32_t> d_pcd_len;
};

namespace mcimpl {
// mc_deskew's body; pcd_len != nullptr: the *_pcd deskew kernels also write each output block's
// ASCII PCD text bytes there (mc_deskew_pcd)
int deskew_call(mc_ctx* c, const mc_batch* in, mc_batch* out, int mode, int pose_select, int32_t* pcd_len);
// the sub-tile order (0 dealt, 1 XCD-contiguous) mc_deskew's kernel takes for this mode and batch
int deskew_order(const mc_ctx* c, const mc_batch* in, int mode);
// The one way to say "this batch's columns were written" (DESIGN.md §4.1 lists who says what).  A
// writer announces kWrotePoints before it queues its launch, so a launch that fails leaves the sums
// stale, and adds kWroteSums once the launch that also wrote them is queued.  kWroteTime marks the
// spans and the rule stale; with kSpansNow they are recomputed in the call (one synchronisation: the
// only way the call fails), else by the next reader (ensure_spans).  kLeftQueued: the caller returns
// with this work still on the stream, which the next k_prep must not overtake.
// kHoldsIntensity, once a deskew of `src` into b is queued: b's intensity column is src's as it stands.
enum : unsigned {
  kWrotePoints = 1, kWroteSums = 2, kWroteTime = 4, kSpansNow = 8, kLeftQueued = 16, kHoldsIntensity = 32
};
// a kernel that writes every column and leaves the stream running: the decoders, the voxel emit
constexpr unsigned kWroteAllQueued = kWrotePoints | kWroteTime | kSpansNow | kLeftQueued;
int batch_columns_written(mc_batch* b, unsigned what, const mc_batch* src = nullptr);
}  // namespace mcimpl
