// codecs.hip — host side of the file codecs in include/mcdeskew.h:
// LVX v1.1 files (LMC:24-272) and ASCII PCD bodies (LMC:932-948) encoded on the device from a
// device-resident (N, ld) float64 AoS cloud; and of the CSIM exports (LVX / LVX2 / LVX3 files,
// CSIM:235-374, and the PCD / XYZ / CSV bodies of DataExporter, CSIM:1603-1715; csim_codecs.hpp); and
// of their inverse, the decoders of those files into device rows or a batch (ingest.hpp, f7); and of
// the LAS 1.2 codec in both directions (las.hpp, f8).
#include "codecs.hpp"
#include "csim_codecs.hpp"
#include "hostutil.hpp"
#include "ingest.hpp"
#include "ingest_index.hpp"
#include "las.hpp"
#include "las_index.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

using namespace mc;

namespace {

// The codecs' state in the context (its codec slot, internal.hpp): made by the first call that needs it.
struct CodecState : mcimpl::CtxExt {
  // per-call frame / unit tables carved from one scratch buffer, error flag
  DevBuf<char> scratch;
  DevBuf<int> err;
  // mc_deskew_pcd: ASCII PCD text bytes per 256-point output block, written by the deskew kernel
  DevBuf<int32_t> pcd_len;
  EventPairs ev;
  ~CodecState() override { ev_destroy(ev); }
};
CodecState& codec_of(mc_ctx* c) { return *ctx_ext<CodecState>(c, mcimpl::kSlotCodec, true); }

int codec_scratch(mc_ctx* c, size_t bytes, char** out) {
  CodecState& s = codec_of(c);
  if (int r = ctx_reserve(c, s.scratch, bytes)) return r;
  if (!s.err) {
    if (int r = s.err.alloc(1)) return r;
  }
  *out = s.scratch;
  return MC_OK;
}

// the 88 bytes ahead of the first frame: public header (LMC:86-101), private header (LMC:104-110),
// device info block (LMC:146-172)
void lvx_file_header(uint8_t h[kLvxFileHdr]) {
  std::memset(h, 0, kLvxFileHdr);
  std::memcpy(h, "livox_tech", 10);
  h[16] = 1; h[17] = 1;
  const uint32_t magic = 0xAC0EA767u, dur = 50;
  std::memcpy(h + 20, &magic, 4);
  std::memcpy(h + 24, &dur, 4);
  h[28] = 1;                                       // device count
  std::memcpy(h + 29, "3GGDJ6K00200101", 15);      // LiDAR SN (16 B, NUL-terminated)
  h[29 + 33] = 1;                                  // device type
}

int check_frames(int32_t F, const int64_t* counts, std::vector<int64_t>& doff) {
  CHECK_ARG(F >= 0, "n_frames must be >= 0");
  CHECK_ARG(F == 0 || counts, "counts is NULL");
  doff.assign((size_t)F + 1, 0);
  for (int32_t f = 0; f < F; ++f) {
    CHECK_ARG(counts[f] >= 0, "negative frame size at frame %d", f);
    CHECK_ARG(counts[f] < ((int64_t)1 << 31), "frame %d has %lld points (the encoders take < 2^31 per frame)", f,
              (long long)counts[f]);
    doff[f + 1] = doff[f] + counts[f];
  }
  return MC_OK;
}

template <typename T>
size_t put(std::vector<uint8_t>& blob, const T* src, size_t n) {
  const size_t at = (blob.size() + 7) & ~size_t(7);
  blob.resize(at + n * sizeof(T));
  if (n) std::memcpy(blob.data() + at, src, n * sizeof(T));
  return at;
}

// where the points come from: a device (N, ld) float64 AoS array or a batch's blocked columns
struct Source {
  const double* aos = nullptr;
  int64_t ld = 4;
  const mc_batch* batch = nullptr;
};

CodecFrames frames_of(const Source& src, const int64_t* d_doff, const int64_t* d_units, int32_t F, int64_t n_units) {
  CodecFrames cf;
  cf.aos = src.aos;
  cf.ld = src.batch ? 4 : src.ld;
  cf.cols = src.batch ? src.batch->d_cols : nullptr;
  cf.C = src.batch ? src.batch->C : 0;
  cf.poff = src.batch ? src.batch->d_poff : nullptr;
  cf.doff = d_doff;
  cf.unit_off = d_units;
  cf.F = F;
  cf.n_units = n_units;
  cf.frames_per_unit = n_units > 0 ? (double)F / (double)n_units : 0.0;
  return cf;
}

int lvx_encode(mc_ctx* c, const Source& src, int32_t F, const int64_t* counts, const uint64_t* frame_ids,
               const uint64_t* ts_ns, const uint8_t* has_int, void* d_out, int64_t out_bytes);
int pcd_encode(mc_ctx* c, const Source& src, int32_t F, const int64_t* counts, void* d_out, int64_t out_bytes,
               int64_t* body_pos, const int32_t* d_measured = nullptr);

}  // namespace

extern "C" {

int mc_lvx_layout(int32_t F, const int64_t* counts, int64_t* pos) {
  CHECK_ARG(pos, "frame_pos is NULL");
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  pos[0] = kLvxFileHdr;
  for (int32_t f = 0; f < F; ++f)
    pos[f + 1] = pos[f] + kLvxFrameHdr + (counts[f] + kLvxPkgPoints - 1) / kLvxPkgPoints * kLvxPkg;
  return MC_OK;
}

int mc_lvx_encode(mc_ctx* c, const double* d_aos, int64_t ld, int32_t F, const int64_t* counts,
                  const uint64_t* frame_ids, const uint64_t* ts_ns, const uint8_t* has_int, void* d_out,
                  int64_t out_bytes) {
  CHECK_ARG(c && d_out, "NULL argument");
  if (ld < 3) return fail(MC_ERR_INDEX, "LVX points need at least 3 columns; got %lld", (long long)ld);
  Source src;
  src.aos = d_aos;
  src.ld = ld;
  return lvx_encode(c, src, F, counts, frame_ids, ts_ns, has_int, d_out, out_bytes);
}

int mc_lvx_encode_batch(mc_ctx* c, const mc_batch* b, const uint64_t* frame_ids, const uint64_t* ts_ns, void* d_out,
                        int64_t out_bytes) {
  CHECK_ARG(c && b && d_out, "NULL argument");
  CHECK_ARG(b->ctx == c, "batch belongs to another context");
  Source src;
  src.batch = b;
  return lvx_encode(c, src, b->F, b->counts.data(), frame_ids, ts_ns, nullptr, d_out, out_bytes);
}

}  // extern "C"

namespace {

int lvx_encode(mc_ctx* c, const Source& src, int32_t F, const int64_t* counts, const uint64_t* frame_ids,
               const uint64_t* ts_ns, const uint8_t* has_int, void* d_out, int64_t out_bytes) {
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  CHECK_ARG(F == 0 || (frame_ids && ts_ns), "frame_ids / timestamp_ns are NULL");
  CHECK_ARG(doff[F] == 0 || src.aos || src.batch, "points pointer is NULL");
  CHECK_ARG(((uintptr_t)d_out & 1) == 0, "d_out must be 2-byte aligned");
  std::vector<int64_t> pos((size_t)F + 1), units((size_t)F + 1, 0);
  mc_lvx_layout(F, counts, pos.data());
  if (out_bytes < pos[F])
    return fail(MC_ERR_SPACE, "LVX output needs %lld bytes, buffer has %lld", (long long)pos[F], (long long)out_bytes);
  for (int32_t f = 0; f < F; ++f) units[f + 1] = units[f] + (counts[f] + kLvxUnitPoints - 1) / kLvxUnitPoints;
  const int64_t n_pkg = units[F];   // units of up to kLvxPkgPerWG packages
  CHECK_ARG(n_pkg < (int64_t)INT32_MAX, "too many packages for one launch");
  DeviceGuard g(c->device);

  std::vector<uint8_t> blob;
  const size_t o_doff = put(blob, doff.data(), doff.size());
  const size_t o_unit = put(blob, units.data(), units.size());
  const size_t o_pos = put(blob, pos.data(), (size_t)F + 1);
  const size_t o_ids = put(blob, frame_ids, (size_t)F);
  const size_t o_ts = put(blob, ts_ns, (size_t)F);
  const size_t o_hi = has_int ? put(blob, has_int, (size_t)F) : 0;
  char* d = nullptr;
  if (int r = codec_scratch(c, blob.size(), &d)) return r;
  HIPCHK(hipMemcpyAsync(d, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
  uint8_t hdr[kLvxFileHdr];
  lvx_file_header(hdr);
  HIPCHK(hipMemcpyAsync(d_out, hdr, kLvxFileHdr, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(codec_of(c).err, 0, sizeof(int), c->stream));

  LvxArgs a;
  a.src = frames_of(src, reinterpret_cast<const int64_t*>(d + o_doff), reinterpret_cast<const int64_t*>(d + o_unit),
                    F, n_pkg);
  a.frame_pos = reinterpret_cast<const int64_t*>(d + o_pos);
  a.frame_id = reinterpret_cast<const uint64_t*>(d + o_ids);
  a.ts_ns = reinterpret_cast<const uint64_t*>(d + o_ts);
  a.has_int = has_int ? reinterpret_cast<const uint8_t*>(d + o_hi) : nullptr;
  a.out = static_cast<char*>(d_out);
  a.err = codec_of(c).err;
  a.order = src.batch ? src.batch->hot_order ^ 1 : 0;   // start where the last kernel over the batch ended
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    // frame headers: each frame's first unit writes its own, so this launch only when a frame has no
    // points (and therefore no unit)
    const bool empty_frame = std::any_of(counts, counts + F, [](int64_t n) { return n == 0; });
    if (F > 0 && empty_frame)
      hipLaunchKernelGGL(k_lvx_frames, dim3((F + kCodecBlock - 1) / kCodecBlock), dim3(kCodecBlock), 0, c->stream,
                         a, (int64_t)0);
    if (n_pkg > 0) {
      hipLaunchKernelGGL(k_lvx_packages, dim3((uint32_t)n_pkg), dim3(kCodecBlock), 0, c->stream, a);
      if (src.batch) src.batch->hot_order = a.order;
    }
  }
  HIPCHK(hipGetLastError());
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, codec_of(c).err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (err) return fail(MC_ERR_INVALID, "cannot convert float NaN to integer (NaN coordinate or intensity)");
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_pcd_encode(mc_ctx* c, const double* d_aos, int64_t ld, int32_t F, const int64_t* counts, void* d_out,
                  int64_t out_bytes, int64_t* body_pos) {
  CHECK_ARG(c && body_pos, "NULL argument");
  if (ld < 4) return fail(MC_ERR_INDEX, "index 3 is out of bounds for axis 0 with size %lld", (long long)ld);
  Source src;
  src.aos = d_aos;
  src.ld = ld;
  return pcd_encode(c, src, F, counts, d_out, out_bytes, body_pos);
}

int mc_pcd_encode_batch(mc_ctx* c, const mc_batch* b, void* d_out, int64_t out_bytes, int64_t* body_pos) {
  CHECK_ARG(c && b && body_pos, "NULL argument");
  CHECK_ARG(b->ctx == c, "batch belongs to another context");
  Source src;
  src.batch = b;
  // MC_BATCH_WITH_PCD_LEN: the kernel that last wrote the columns left their text sums (no measure pass)
  return pcd_encode(c, src, b->F, b->counts.data(), d_out, out_bytes, body_pos,
                    b->state.sums_current() ? b->d_pcd_len : nullptr);
}

int mc_deskew_pcd(mc_ctx* c, const mc_batch* in, mc_batch* out, int mode, int pose_select, void* d_out,
                  int64_t out_bytes, int64_t* body_pos) {
  CHECK_ARG(c && in && out && body_pos, "NULL argument");
  CHECK_ARG(out != in, "mc_deskew_pcd needs an output batch other than the input");
  CHECK_ARG(out->ctx == c, "batch belongs to another context");
  DeviceGuard g(c->device);
  if (out->d_pcd_len) {   // MC_BATCH_WITH_PCD_LEN: the deskew writes the batch's own sums
    if (int r = mcimpl::deskew_call(c, in, out, mode, pose_select, nullptr)) return r;
    return mc_pcd_encode_batch(c, out, d_out, out_bytes, body_pos);
  }
  // one text-byte slot per 256-point block of the output batch (= one PCD tile)
  const int64_t blocks = out->P / kBlkPts;
  if (int r = ctx_reserve(c, codec_of(c).pcd_len, (size_t)blocks)) return r;
  if (int r = mcimpl::deskew_call(c, in, out, mode, pose_select, blocks > 0 ? codec_of(c).pcd_len.get() : nullptr)) return r;
  Source src;
  src.batch = out;
  return pcd_encode(c, src, out->F, out->counts.data(), d_out, out_bytes, body_pos, codec_of(c).pcd_len);
}

}  // extern "C"

namespace {

// d_measured (mc_deskew_pcd): the tiles' text bytes already written by the deskew kernel that
// produced the batch (pcd_value_len sums per 256-point block = per tile); the measure pass is then
// skipped unless a tile holds a value outside the packed path, whose exact length only the measure
// pass forms.
int pcd_encode(mc_ctx* c, const Source& src, int32_t F, const int64_t* counts, void* d_out, int64_t out_bytes,
               int64_t* body_pos, const int32_t* d_measured) {
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  CHECK_ARG(doff[F] == 0 || src.aos || src.batch, "points pointer is NULL");
  std::vector<int64_t> units((size_t)F + 1, 0);
  for (int32_t f = 0; f < F; ++f) units[f + 1] = units[f] + (counts[f] + kPcdBlock - 1) / kPcdBlock;
  const int64_t n_tiles = units[F];
  CHECK_ARG(n_tiles < (int64_t)INT32_MAX, "too many tiles for one launch");
  if (n_tiles == 0) {
    std::fill(body_pos, body_pos + F + 1, (int64_t)0);
    return MC_OK;
  }
  DeviceGuard g(c->device);
  std::vector<uint8_t> blob;
  const size_t o_doff = put(blob, doff.data(), doff.size());
  const size_t o_unit = put(blob, units.data(), units.size());
  const size_t o_tb = put(blob, (const int32_t*)nullptr, 0);
  blob.resize(o_tb + (size_t)n_tiles * sizeof(int32_t));
  const size_t o_tp = put(blob, (const int64_t*)nullptr, 0);
  blob.resize(o_tp + (size_t)n_tiles * sizeof(int64_t));
  char* d = nullptr;
  if (int r = codec_scratch(c, blob.size(), &d)) return r;
  HIPCHK(hipMemcpyAsync(d, blob.data(), o_tb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(codec_of(c).err, 0, sizeof(int), c->stream));
  PcdArgs a;
  a.src = frames_of(src, reinterpret_cast<const int64_t*>(d + o_doff), reinterpret_cast<const int64_t*>(d + o_unit),
                    F, n_tiles);
  a.tile_bytes = reinterpret_cast<int32_t*>(d + o_tb);
  a.tile_pos = reinterpret_cast<const int64_t*>(d + o_tp);
  a.out = static_cast<char*>(d_out);
  a.err = codec_of(c).err;
  // batch source: each pass starts where the previous kernel over the batch ended (stream_unit);
  // fused (d_measured): the write pass follows the deskew kernel directly
  const int hot = src.batch ? src.batch->hot_order : 1;
  a.morder = hot ^ 1;
  a.worder = hot ^ 1;
  std::vector<int32_t> tb((size_t)n_tiles);
  bool measured = false;
  if (d_measured) {
    HIPCHK(hipMemcpyAsync(tb.data(), d_measured, tb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    measured = std::all_of(tb.begin(), tb.end(), [](int32_t v) { return v >= 0 && v < kPcdSlowValue; });
    if (measured) a.tile_bytes = const_cast<int32_t*>(d_measured);   // the write pass reads it (no slow flags)
  }
  if (!measured) {
    a.worder = a.morder ^ 1;
    {
      TimedRegion tr(c, &codec_of(c).ev, c->stream);
      const int per = a.src.cols ? kPcdMeasureTiles : kPcdTilesPerWG;   // tiles per measure workgroup
      const dim3 mgrid((uint32_t)((n_tiles + per - 1) / per));
      if (a.src.cols) hipLaunchKernelGGL(k_pcd_measure<true>, mgrid, dim3(kPcdBlock), 0, c->stream, a);
      else hipLaunchKernelGGL(k_pcd_measure<false>, mgrid, dim3(kPcdBlock), 0, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tb.data(), a.tile_bytes, tb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (a.src.cols) {
      // the float32 measure pass only flags tiles with lines outside the packed path: their exact
      // bytes from k_pcd_measure_list (the list rides in the tile-position slots, not yet written)
      HIPCHK(hipStreamSynchronize(c->stream));
      std::vector<int32_t> flagged;
      for (int64_t t = 0; t < n_tiles; ++t)
        if (tb[t] & kPcdSlowTile) flagged.push_back((int32_t)t);
      if (!flagged.empty()) {
        int32_t* d_list = reinterpret_cast<int32_t*>(d + o_tp);
        HIPCHK(hipMemcpyAsync(d_list, flagged.data(), flagged.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                              c->stream));
        {
          TimedRegion tr(c, &codec_of(c).ev, c->stream);
          hipLaunchKernelGGL(k_pcd_measure_list, dim3((uint32_t)flagged.size()), dim3(kPcdBlock), 0, c->stream, a,
                             (const int32_t*)d_list);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tb.data(), a.tile_bytes, tb.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                              c->stream));
      }
    }
  }
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, codec_of(c).err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (err) return fail(MC_ERR_INVALID, "a value has |v| >= 2^107, beyond the device %%.6f formatter");
  // tiles holding a line outside the packed path (kPcdSlowTile) go to the byte-path kernel
  std::vector<int64_t> tpos((size_t)n_tiles);
  std::vector<int32_t> slow;
  int64_t run = 0;
  for (int32_t f = 0; f < F; ++f) {
    body_pos[f] = run;
    for (int64_t t = units[f]; t < units[f + 1]; ++t) {
      if (tb[t] & kPcdSlowTile) slow.push_back((int32_t)t);
      tpos[t] = run;
      run += tb[t] & ~kPcdSlowTile;
    }
  }
  body_pos[F] = run;
  if (out_bytes < run)
    return fail(MC_ERR_SPACE, "PCD text needs %lld bytes, buffer has %lld", (long long)run, (long long)out_bytes);
  CHECK_ARG(d_out, "d_out is NULL");
  HIPCHK(hipMemcpyAsync(d + o_tp, tpos.data(), tpos.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  const dim3 grid((uint32_t)((n_tiles + kPcdWriteTiles - 1) / kPcdWriteTiles));
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    if (a.src.cols) hipLaunchKernelGGL(k_pcd_write<true>, grid, dim3(kPcdBlock), 0, c->stream, a);
    else hipLaunchKernelGGL(k_pcd_write<false>, grid, dim3(kPcdBlock), 0, c->stream, a);
  }
  if (src.batch) src.batch->hot_order = a.worder;
  HIPCHK(hipGetLastError());
  if (!slow.empty()) {
    // the list rides in the scratch blob's tile-byte slots, which k_pcd_write has finished reading
    // (same stream); the byte path reads no tile bytes
    HIPCHK(hipMemcpyAsync(a.tile_bytes, slow.data(), slow.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                          c->stream));
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    hipLaunchKernelGGL(k_pcd_write_bytes, dim3((uint32_t)slow.size()), dim3(kPcdBlock), 0, c->stream, a,
                       (const int32_t*)a.tile_bytes);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

}  // namespace

// ---- CSIM exports: LivoxLVXWriter.write_lvx_file (CSIM:235-374), DataExporter (CSIM:1603-1715) -----
namespace {

int csim_version(int version, int* ver) {
  CHECK_ARG(version == MC_CSIM_LVX_LEGACY || version == MC_CSIM_LVX2 || version == MC_CSIM_LVX3,
            "Unsupported format version: %d", version);
  *ver = version == MC_CSIM_LVX_LEGACY ? 1 : 2;   // lvx3 writes lvx2's bytes (CSIM:289-293)
  return MC_OK;
}

int csim_batch_source(mc_ctx* c, const mc_batch* b, Source* src) {
  CHECK_ARG(c && b, "NULL argument");
  CHECK_ARG(b->ctx == c, "batch belongs to another context");
  if (!b->has_t()) return fail(MC_ERR_STATE, "the CSIM encoders need a batch created with MC_BATCH_WITH_TIME");
  if (!b->state.has_frame_starts()) return fail(MC_ERR_STATE, "the batch's frame starts are not set (mc_batch_set_frame_start_ns)");
  src->batch = b;
  return MC_OK;
}

CsimSrc csim_src(const Source& src, const CodecFrames& fr, const uint8_t* d_tags) {
  CsimSrc s;
  s.fr = fr;
  s.fr.ld = src.batch ? 5 : src.ld;
  s.fstart = src.batch ? src.batch->d_frame_start : nullptr;
  s.tags = d_tags;
  return s;
}

struct CsimDevice {
  const uint8_t* sn;   // 16 bytes
  uint8_t type, extrinsic;
  const float* ext;    // roll, pitch, yaw, x, y, z
};

// the bytes ahead of the first frame; -> their count
int csim_file_header(int ver, int32_t F, const CsimDevice& dv, uint8_t h[kCsimLvx2FileHdr]) {
  std::memset(h, 0, kCsimLvx2FileHdr);
  if (ver == 1) {   // CSIM:295-306
    std::memcpy(h, "livox_file", 10);
    const uint32_t one = 1, n = (uint32_t)F;
    std::memcpy(h + 10, &one, 4);
    std::memcpy(h + 14, &n, 4);
    std::memcpy(h + 28, dv.sn, 16);
    h[44] = dv.type;
    return kCsimLvx1FileHdr;
  }
  std::memcpy(h, "livox_tech", 10);   // CSIM:272-280, 323-341
  std::memcpy(h + 10, "2.0.0", 5);
  const uint32_t magic = 0xAC0EA767u, dur = 50, ndev = 1;
  std::memcpy(h + 16, &magic, 4);
  std::memcpy(h + 24, &dur, 4);
  std::memcpy(h + 28, &ndev, 4);
  std::memcpy(h + 32, dv.sn, 16);
  h[48] = dv.type;
  h[49] = dv.extrinsic ? 1 : 0;
  std::memcpy(h + 50, dv.ext, 24);
  return kCsimLvx2FileHdr;
}

int csim_layout(int ver, int32_t F, const int64_t* counts, int64_t* pos) {
  const int fh = ver == 1 ? kCsimLvx1FrameHdr : kCsimLvx2FrameHdr;
  pos[0] = ver == 1 ? kCsimLvx1FileHdr : kCsimLvx2FileHdr;
  for (int32_t f = 0; f < F; ++f) pos[f + 1] = pos[f] + fh + counts[f] * kCsimRec;
  return MC_OK;
}

int csim_lvx_encode(mc_ctx* c, int version, const Source& src, int32_t F, const int64_t* counts, const uint64_t* ts_ns,
                    const uint8_t* d_tags, const CsimDevice& dv, void* d_out, int64_t out_bytes) {
  int ver = 0;
  if (int r = csim_version(version, &ver)) return r;
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  CHECK_ARG(d_out, "d_out is NULL");
  CHECK_ARG(F == 0 || ts_ns, "timestamp_ns is NULL");
  CHECK_ARG(dv.sn && dv.ext, "device info is NULL");
  CHECK_ARG(doff[F] == 0 || src.aos || src.batch, "points pointer is NULL");
  std::vector<int64_t> pos((size_t)F + 1), units((size_t)F + 1, 0);
  csim_layout(ver, F, counts, pos.data());
  if (out_bytes < pos[F])
    return fail(MC_ERR_SPACE, "LVX output needs %lld bytes, buffer has %lld", (long long)pos[F], (long long)out_bytes);
  for (int32_t f = 0; f < F; ++f) units[f + 1] = units[f] + (counts[f] + kCsimUnitPoints - 1) / kCsimUnitPoints;
  const int64_t n_units = units[F];
  CHECK_ARG(n_units < (int64_t)INT32_MAX, "too many units for one launch");
  DeviceGuard g(c->device);

  std::vector<uint8_t> blob;
  const size_t o_doff = put(blob, doff.data(), doff.size());
  const size_t o_unit = put(blob, units.data(), units.size());
  const size_t o_pos = put(blob, pos.data(), (size_t)F + 1);
  const size_t o_ts = put(blob, ts_ns, (size_t)F);
  char* d = nullptr;
  if (int r = codec_scratch(c, blob.size(), &d)) return r;
  HIPCHK(hipMemcpyAsync(d, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
  uint8_t hdr[kCsimLvx2FileHdr];
  const int hb = csim_file_header(ver, F, dv, hdr);
  HIPCHK(hipMemcpyAsync(d_out, hdr, hb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(codec_of(c).err, 0, sizeof(int), c->stream));

  CsimLvxArgs a;
  a.src = csim_src(src, frames_of(src, reinterpret_cast<const int64_t*>(d + o_doff),
                                  reinterpret_cast<const int64_t*>(d + o_unit), F, n_units), d_tags);
  a.frame_pos = reinterpret_cast<const int64_t*>(d + o_pos);
  a.ts_ns = reinterpret_cast<const uint64_t*>(d + o_ts);
  a.out = static_cast<char*>(d_out);
  a.err = codec_of(c).err;
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    const bool empty_frame = std::any_of(counts, counts + F, [](int64_t n) { return n == 0; });
    const dim3 fgrid((F + kCodecBlock - 1) / kCodecBlock), ugrid((uint32_t)n_units), blk(kCodecBlock);
    if (F > 0 && empty_frame) {
      if (ver == 1) hipLaunchKernelGGL(k_csim_lvx_frames<1>, fgrid, blk, 0, c->stream, a);
      else hipLaunchKernelGGL(k_csim_lvx_frames<2>, fgrid, blk, 0, c->stream, a);
    }
    if (n_units > 0) {
      if (ver == 1) hipLaunchKernelGGL(k_csim_lvx<1>, ugrid, blk, 0, c->stream, a);
      else hipLaunchKernelGGL(k_csim_lvx<2>, ugrid, blk, 0, c->stream, a);
    }
  }
  HIPCHK(hipGetLastError());
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, codec_of(c).err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (err)
    return fail(MC_ERR_INVALID, ver == 1 ? "a coordinate overflows float32, or an intensity is NaN or outside 0..255"
                                         : "a coordinate is NaN or infinite, int(v * 1000) is outside int32, or an "
                                           "intensity is NaN or outside 0..255");
  return MC_OK;
}

int csim_text_encode(mc_ctx* c, int format, const Source& src, int32_t F, const int64_t* counts, void* d_out,
                     int64_t out_bytes, int64_t* body_pos) {
  CsimLine line;
  switch (format) {
    case MC_CSIM_PCD: line = {5, ' ', 0x18u, 0}; break;   // CSIM:1664
    case MC_CSIM_XYZ: line = {3, ' ', 0u, 0}; break;      // CSIM:1703
    case MC_CSIM_CSV: line = {5, ',', 0u, 1}; break;      // CSIM:1711-1712
    default: return fail(MC_ERR_INVALID, "unknown CSIM text format %d", format);
  }
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  CHECK_ARG(doff[F] == 0 || src.aos || src.batch, "points pointer is NULL");
  std::vector<int64_t> units((size_t)F + 1, 0);
  for (int32_t f = 0; f < F; ++f) units[f + 1] = units[f] + (counts[f] + kPcdBlock - 1) / kPcdBlock;
  const int64_t n_tiles = units[F];
  CHECK_ARG(n_tiles < (int64_t)INT32_MAX, "too many tiles for one launch");
  if (n_tiles == 0) {
    std::fill(body_pos, body_pos + F + 1, (int64_t)0);
    return MC_OK;
  }
  DeviceGuard g(c->device);
  std::vector<uint8_t> blob;
  const size_t o_doff = put(blob, doff.data(), doff.size());
  const size_t o_unit = put(blob, units.data(), units.size());
  const size_t o_tb = put(blob, (const int32_t*)nullptr, 0);
  blob.resize(o_tb + (size_t)n_tiles * sizeof(int32_t));
  const size_t o_tp = put(blob, (const int64_t*)nullptr, 0);
  blob.resize(o_tp + (size_t)n_tiles * sizeof(int64_t));
  char* d = nullptr;
  if (int r = codec_scratch(c, blob.size(), &d)) return r;
  HIPCHK(hipMemcpyAsync(d, blob.data(), o_tb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(codec_of(c).err, 0, sizeof(int), c->stream));
  CsimTextArgs a;
  a.src = csim_src(src, frames_of(src, reinterpret_cast<const int64_t*>(d + o_doff),
                                  reinterpret_cast<const int64_t*>(d + o_unit), F, n_tiles), nullptr);
  a.line = line;
  a.tile_bytes = reinterpret_cast<int32_t*>(d + o_tb);
  a.tile_pos = reinterpret_cast<const int64_t*>(d + o_tp);
  a.out = static_cast<char*>(d_out);
  a.err = codec_of(c).err;
  const dim3 grid((uint32_t)n_tiles), blk(kPcdBlock);
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    if (line.ncols == 3) hipLaunchKernelGGL(k_csim_text_measure<3>, grid, blk, 0, c->stream, a);
    else hipLaunchKernelGGL(k_csim_text_measure<5>, grid, blk, 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  std::vector<int32_t> tb((size_t)n_tiles);
  int err = 0;
  HIPCHK(hipMemcpyAsync(tb.data(), a.tile_bytes, tb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&err, codec_of(c).err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (err) return fail(MC_ERR_INVALID, "a value has |v| >= 2^107, beyond the device %%.6f / %%.0f formatters");
  std::vector<int64_t> tpos((size_t)n_tiles);
  int64_t run = 0;
  for (int32_t f = 0; f < F; ++f) {
    body_pos[f] = run;
    for (int64_t t = units[f]; t < units[f + 1]; ++t) { tpos[t] = run; run += tb[t]; }
  }
  body_pos[F] = run;
  if (out_bytes < run)
    return fail(MC_ERR_SPACE, "the text needs %lld bytes, buffer has %lld", (long long)run, (long long)out_bytes);
  CHECK_ARG(d_out, "d_out is NULL");
  HIPCHK(hipMemcpyAsync(d + o_tp, tpos.data(), tpos.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    if (line.ncols == 3) hipLaunchKernelGGL(k_csim_text_write<3>, grid, blk, 0, c->stream, a);
    else hipLaunchKernelGGL(k_csim_text_write<5>, grid, blk, 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_csim_lvx_layout(int version, int32_t F, const int64_t* counts, int64_t* pos) {
  int ver = 0;
  if (int r = csim_version(version, &ver)) return r;
  CHECK_ARG(pos, "frame_pos is NULL");
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  return csim_layout(ver, F, counts, pos);
}

int mc_csim_lvx_encode(mc_ctx* c, int version, const double* d_rows, int64_t ld, int32_t F, const int64_t* counts,
                       const uint64_t* ts_ns, const uint8_t* d_tags, const uint8_t* lidar_sn, uint8_t device_type,
                       uint8_t extrinsic_enable, const float* extrinsics, void* d_out, int64_t out_bytes) {
  CHECK_ARG(c, "ctx is NULL");
  if (ld < 5) return fail(MC_ERR_INDEX, "CSIM rows are x, y, z, intensity, timestamp: ld >= 5; got %lld", (long long)ld);
  Source src;
  src.aos = d_rows;
  src.ld = ld;
  return csim_lvx_encode(c, version, src, F, counts, ts_ns, d_tags, {lidar_sn, device_type, extrinsic_enable, extrinsics},
                         d_out, out_bytes);
}

int mc_csim_lvx_encode_batch(mc_ctx* c, int version, const mc_batch* b, const uint64_t* ts_ns, const uint8_t* d_tags,
                             const uint8_t* lidar_sn, uint8_t device_type, uint8_t extrinsic_enable,
                             const float* extrinsics, void* d_out, int64_t out_bytes) {
  Source src;
  if (int r = csim_batch_source(c, b, &src)) return r;
  return csim_lvx_encode(c, version, src, b->F, b->counts.data(), ts_ns, d_tags,
                         {lidar_sn, device_type, extrinsic_enable, extrinsics}, d_out, out_bytes);
}

int mc_csim_text_encode(mc_ctx* c, int format, const double* d_rows, int64_t ld, int32_t F, const int64_t* counts,
                        void* d_out, int64_t out_bytes, int64_t* body_pos) {
  CHECK_ARG(c && body_pos, "NULL argument");
  if (ld < 5) return fail(MC_ERR_INDEX, "CSIM rows are x, y, z, intensity, timestamp: ld >= 5; got %lld", (long long)ld);
  Source src;
  src.aos = d_rows;
  src.ld = ld;
  return csim_text_encode(c, format, src, F, counts, d_out, out_bytes, body_pos);
}

int mc_csim_text_encode_batch(mc_ctx* c, int format, const mc_batch* b, void* d_out, int64_t out_bytes,
                              int64_t* body_pos) {
  CHECK_ARG(body_pos, "NULL argument");
  Source src;
  if (int r = csim_batch_source(c, b, &src)) return r;
  return csim_text_encode(c, format, src, b->F, b->counts.data(), d_out, out_bytes, body_pos);
}

}  // extern "C"

// ---- ingest (f7): LVX files and ASCII PCD / XYZ / CSV text back into device rows or a batch ----------
namespace {

int ingest_fail(const char* msg) { return fail(MC_ERR_INVALID, "%s", msg); }

int lvx_decode(mc_ctx* c, int format, const void* d_file, int64_t bytes, int32_t F, const int64_t* frame_pos,
               const int64_t* counts, const int64_t* ts_ns, int64_t period, double* d_rows, int64_t ld, mc_batch* out,
               uint8_t* d_tags) {
  CHECK_ARG(c && d_file, "NULL argument");
  CHECK_ARG(((uintptr_t)d_file & 15) == 0, "d_file must be 16-byte aligned (and padded to a multiple of 16 bytes)");
  char msg[256];
  if (mcingest::check_layout(format, bytes, F, frame_pos, counts, msg, sizeof msg)) return ingest_fail(msg);
  CHECK_ARG(F == 0 || counts, "counts is NULL");
  CHECK_ARG(format == MC_LVX_V11 || F == 0 || ts_ns, "timestamp_ns is NULL");
  std::vector<int64_t> doff;
  if (int r = check_frames(F, counts, doff)) return r;
  std::vector<int64_t> units((size_t)F + 1, 0);
  for (int32_t f = 0; f < F; ++f) units[f + 1] = units[f] + (counts[f] + kIngestUnit - 1) / kIngestUnit;
  const int64_t n_units = units[F];
  CHECK_ARG(n_units < (int64_t)INT32_MAX, "too many units for one launch");
  if (out) {
    CHECK_ARG(out->ctx == c, "batch belongs to another context");
    if (!out->has_t()) return fail(MC_ERR_STATE, "mc_lvx_decode_batch needs a batch created with MC_BATCH_WITH_TIME");
    CHECK_ARG(out->F == F && std::equal(counts, counts + F, out->counts.begin()),
              "the batch's frame counts differ from the decoded counts");
    CHECK_ARG(period >= 0, "point_period_ns must be >= 0");
    for (int32_t f = 0; f < F; ++f)
      CHECK_ARG(counts[f] <= 1 || (unsigned __int128)period * (uint64_t)(counts[f] - 1) <= (uint64_t)INT32_MAX,
                "frame %d: t_ns = index x point_period_ns exceeds int32 nanoseconds", f);
    CHECK_ARG(F == 0 || ts_ns, "timestamp_ns is NULL");
  } else {
    CHECK_ARG(doff[F] == 0 || d_rows, "d_rows is NULL");
  }
  DeviceGuard g(c->device);
  if (out)
    if (int r = mc_batch_set_frame_start_ns(out, ts_ns)) return r;
  if (n_units == 0) return MC_OK;

  std::vector<uint8_t> blob;
  const size_t o_doff = put(blob, doff.data(), doff.size());
  const size_t o_unit = put(blob, units.data(), units.size());
  const size_t o_pos = put(blob, frame_pos, (size_t)F + 1);
  const size_t o_ts = ts_ns ? put(blob, ts_ns, (size_t)F) : 0;
  char* d = nullptr;
  if (int r = codec_scratch(c, blob.size(), &d)) return r;
  HIPCHK(hipMemcpyAsync(d, blob.data(), blob.size(), hipMemcpyHostToDevice, c->stream));
  LvxInArgs a;
  Source none;
  a.fr = frames_of(none, reinterpret_cast<const int64_t*>(d + o_doff), reinterpret_cast<const int64_t*>(d + o_unit), F,
                   n_units);
  a.fr.poff = out ? out->d_poff : nullptr;
  a.file = static_cast<const uint8_t*>(d_file);
  a.frame_pos = reinterpret_cast<const int64_t*>(d + o_pos);
  a.ts_ns = ts_ns ? reinterpret_cast<const int64_t*>(d + o_ts) : nullptr;
  a.period = period;
  a.rows = d_rows;
  a.ld = ld;
  a.cols = out ? out->d_cols : nullptr;
  a.tags = d_tags;
  const dim3 grid((uint32_t)n_units), blk(kCodecBlock);
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    if (out) {
      if (format == MC_LVX_V11) hipLaunchKernelGGL((k_lvx_decode<0, true>), grid, blk, 0, c->stream, a);
      else if (format == MC_CSIM_LVX_LEGACY) hipLaunchKernelGGL((k_lvx_decode<1, true>), grid, blk, 0, c->stream, a);
      else hipLaunchKernelGGL((k_lvx_decode<2, true>), grid, blk, 0, c->stream, a);
    } else {
      if (format == MC_LVX_V11) hipLaunchKernelGGL((k_lvx_decode<0, false>), grid, blk, 0, c->stream, a);
      else if (format == MC_CSIM_LVX_LEGACY) hipLaunchKernelGGL((k_lvx_decode<1, false>), grid, blk, 0, c->stream, a);
      else hipLaunchKernelGGL((k_lvx_decode<2, false>), grid, blk, 0, c->stream, a);
    }
  }
  HIPCHK(hipGetLastError());
  if (out)
    if (int r = mcimpl::batch_columns_written(out, mcimpl::kWroteAllQueued)) return r;
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

// the count pass: lines starting in each 4096-byte tile -> tile_off (exclusive prefix, host) and the total
int text_count(mc_ctx* c, const void* d_text, int64_t bytes, std::vector<int64_t>& tile_off, int64_t* n_lines) {
  CHECK_ARG(c && n_lines, "NULL argument");
  CHECK_ARG(bytes >= 0, "negative size");
  CHECK_ARG(bytes == 0 || d_text, "d_text is NULL");
  CHECK_ARG(((uintptr_t)d_text & 15) == 0, "d_text must be 16-byte aligned (and padded to a multiple of 16 bytes)");
  const int64_t T = (bytes + kTextTile - 1) / kTextTile;
  CHECK_ARG(T < (int64_t)INT32_MAX, "text too large for one launch");
  tile_off.assign((size_t)T + 1, 0);
  if (T == 0) { *n_lines = 0; return MC_OK; }
  char* d = nullptr;
  if (int r = codec_scratch(c, (size_t)T * sizeof(int32_t), &d)) return r;
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    hipLaunchKernelGGL(k_text_count, dim3((uint32_t)T), dim3(kPcdBlock), 0, c->stream, static_cast<const char*>(d_text),
                       bytes, reinterpret_cast<int32_t*>(d));
  }
  HIPCHK(hipGetLastError());
  std::vector<int32_t> tc((size_t)T);
  HIPCHK(hipMemcpyAsync(tc.data(), d, tc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t t = 0; t < T; ++t) tile_off[t + 1] = tile_off[t] + tc[t];
  *n_lines = tile_off[T];
  return MC_OK;
}

int text_decode(mc_ctx* c, int sep, int32_t n_cols, const void* d_text, int64_t bytes, int64_t n_lines, double* d_rows,
                int64_t ld, mc_batch* out, const int64_t* frame_start_ns, int64_t* frame_start_out, int64_t* bad_line) {
  CHECK_ARG(c, "ctx is NULL");
  CHECK_ARG(sep == ' ' || sep == ',', "the separator is ' ' (PCD, XYZ) or ',' (CSV)");
  CHECK_ARG(n_cols >= 3 && n_cols <= kIngestMaxCols, "3 to %d columns; got %d", kIngestMaxCols, n_cols);
  if (bad_line) *bad_line = 0;
  DeviceGuard g(c->device);
  std::vector<int64_t> tile_off;
  int64_t counted = 0;
  if (int r = text_count(c, d_text, bytes, tile_off, &counted)) return r;
  const bool with_t = out && out->has_t() && n_cols >= 5;
  if (out) {
    CHECK_ARG(out->ctx == c, "batch belongs to another context");
    CHECK_ARG(out->N == counted, "the batch holds %lld points, the text %lld lines", (long long)out->N,
              (long long)counted);
    if (n_cols >= 5 && !out->has_t())
      return fail(MC_ERR_STATE, "a text with a timestamp column needs a batch created with MC_BATCH_WITH_TIME");
  } else {
    CHECK_ARG(n_lines == counted, "the text holds %lld lines, not %lld", (long long)counted, (long long)n_lines);
    if (ld < n_cols) return fail(MC_ERR_INDEX, "rows of %d columns need ld >= %d; got %lld", n_cols, n_cols, (long long)ld);
    CHECK_ARG(counted == 0 || d_rows, "d_rows is NULL");
  }
  if (counted == 0) {
    if (out && out->has_t()) {
      std::vector<int64_t> z((size_t)out->F, 0);
      if (int r = mc_batch_set_frame_start_ns(out, frame_start_ns ? frame_start_ns : z.data())) return r;
      if (frame_start_out) std::copy_n(frame_start_ns ? frame_start_ns : z.data(), out->F, frame_start_out);
    }
    return MC_OK;
  }
  const int64_t T = (int64_t)tile_off.size() - 1, PT = (counted + kTextLines - 1) / kTextLines;
  CHECK_ARG(PT < (int64_t)INT32_MAX, "too many lines for one launch");
  // scratch: tile_off[T] | starts[n + 1] | flags[PT]
  const size_t o_off = 0, o_st = o_off + (size_t)T * 8, o_fl = o_st + ((size_t)counted + 1) * 8;
  char* d = nullptr;
  if (int r = codec_scratch(c, o_fl + (size_t)PT * 4, &d)) return r;
  HIPCHK(hipMemcpyAsync(d + o_off, tile_off.data(), (size_t)T * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d + o_st + (size_t)counted * 8, &bytes, 8, hipMemcpyHostToDevice, c->stream));
  TextArgs a;
  a.text = static_cast<const char*>(d_text);
  a.bytes = bytes;
  a.starts = reinterpret_cast<const int64_t*>(d + o_st);
  a.n_lines = counted;
  a.n_cols = n_cols;
  a.sep = sep;
  a.rows = d_rows;
  a.ld = ld;
  a.cols = out ? out->d_cols : nullptr;
  a.C = out ? out->C : 0;
  a.doff = out ? out->d_doff : nullptr;
  a.poff = out ? out->d_poff : nullptr;
  a.F = out ? out->F : 0;
  a.fstart = out ? out->d_frame_start : nullptr;
  a.tile_flag = reinterpret_cast<uint32_t*>(d + o_fl);
  if (with_t && frame_start_ns)
    if (int r = mc_batch_set_frame_start_ns(out, frame_start_ns)) return r;
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    hipLaunchKernelGGL(k_text_starts, dim3((uint32_t)T), dim3(kPcdBlock), 0, c->stream, a.text, bytes,
                       reinterpret_cast<const int64_t*>(d + o_off), reinterpret_cast<int64_t*>(d + o_st));
    if (with_t && !frame_start_ns && out->F > 0)
      hipLaunchKernelGGL(k_text_frame_start, dim3((out->F + kPcdBlock - 1) / kPcdBlock), dim3(kPcdBlock), 0, c->stream, a);
    if (out) hipLaunchKernelGGL(k_text_parse<true>, dim3((uint32_t)PT), dim3(kPcdBlock), 0, c->stream, a);
    else hipLaunchKernelGGL(k_text_parse<false>, dim3((uint32_t)PT), dim3(kPcdBlock), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> flags((size_t)PT);
  HIPCHK(hipMemcpyAsync(flags.data(), a.tile_flag, flags.size() * 4, hipMemcpyDeviceToHost, c->stream));
  if (out) {
    if (with_t && !frame_start_ns) {
      std::vector<int64_t> fs((size_t)out->F);
      HIPCHK(hipMemcpyAsync(fs.data(), out->d_frame_start, fs.size() * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      out->state.frame_starts_set();   // (the kernel wrote them)
      if (frame_start_out) std::copy(fs.begin(), fs.end(), frame_start_out);
    } else if (with_t && frame_start_out) {
      std::copy_n(frame_start_ns, out->F, frame_start_out);
    }
    if (int r = mcimpl::batch_columns_written(out, mcimpl::kWroteAllQueued)) return r;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t t = 0; t < PT; ++t) {
    if (flags[t] == 0xffffffffu) continue;
    const int64_t line = t * kTextLines + (flags[t] >> 2) + 1;
    if (bad_line) *bad_line = line;
    switch (flags[t] & 3u) {
      case kIngestBadFields:
        return fail(MC_ERR_INVALID, "line %lld does not hold %d fields", (long long)line, n_cols);
      case kIngestBadTime:
        return fail(MC_ERR_INVALID, "line %lld: the timestamp minus its frame start does not fit int32 nanoseconds",
                    (long long)line);
      default:
        return fail(MC_ERR_INVALID,
                    "line %lld holds a token beyond the device parser ([+-]digits[.digits] with at most 19 "
                    "significant and 19 fractional digits, nan, inf)", (long long)line);
    }
  }
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_lvx_probe(const void* file, int64_t bytes, int* format, int32_t* n_frames) {
  char msg[256];
  if (mcingest::probe(static_cast<const uint8_t*>(file), bytes, format, n_frames, msg, sizeof msg)) return ingest_fail(msg);
  return MC_OK;
}

int mc_lvx_index(const void* file, int64_t bytes, int format, int32_t n_frames, int64_t* frame_pos, int64_t* slots,
                 uint64_t* frame_ids, int64_t* timestamp_ns, uint8_t* lidar_sn, uint8_t* device_type,
                 uint8_t* extrinsic_enable, float* extrinsics) {
  char msg[256];
  mcingest::DeviceBlock dv;
  if (mcingest::index(static_cast<const uint8_t*>(file), bytes, format, n_frames, frame_pos, slots, frame_ids,
                      timestamp_ns, &dv, msg, sizeof msg))
    return ingest_fail(msg);
  if (lidar_sn) std::memcpy(lidar_sn, dv.sn, 16);
  if (device_type) *device_type = dv.device_type;
  if (extrinsic_enable) *extrinsic_enable = dv.extrinsic_enable;
  if (extrinsics) std::memcpy(extrinsics, dv.extrinsics, sizeof dv.extrinsics);
  return MC_OK;
}

int mc_lvx_count(mc_ctx* c, int format, const void* d_file, int64_t bytes, int32_t F, const int64_t* frame_pos,
                 const int64_t* slots, int keep_padding, int64_t* counts_out) {
  CHECK_ARG(c && counts_out, "NULL argument");
  CHECK_ARG(F == 0 || slots, "slots is NULL");
  char msg[256];
  if (mcingest::check_layout(format, bytes, F, frame_pos, slots, msg, sizeof msg)) return ingest_fail(msg);
  if (format != MC_LVX_V11 || keep_padding || F == 0) {
    std::copy_n(slots, F, counts_out);
    return MC_OK;
  }
  CHECK_ARG(d_file, "d_file is NULL");
  DeviceGuard g(c->device);
  const size_t o_cnt = ((size_t)F + 1) * 8;
  char* d = nullptr;
  if (int r = codec_scratch(c, o_cnt + (size_t)F * 8, &d)) return r;
  HIPCHK(hipMemcpyAsync(d, frame_pos, ((size_t)F + 1) * 8, hipMemcpyHostToDevice, c->stream));
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    hipLaunchKernelGGL(k_lvx_trim, dim3((F + 3) / 4), dim3(kCodecBlock), 0, c->stream,
                       static_cast<const uint8_t*>(d_file), reinterpret_cast<const int64_t*>(d), F,
                       reinterpret_cast<int64_t*>(d + o_cnt));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(counts_out, d + o_cnt, (size_t)F * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

int mc_lvx_decode(mc_ctx* c, int format, const void* d_file, int64_t bytes, int32_t F, const int64_t* frame_pos,
                  const int64_t* counts, const int64_t* timestamp_ns, int64_t point_period_ns, double* d_rows,
                  int64_t ld, uint8_t* d_tags) {
  if (ld < 5) return fail(MC_ERR_INDEX, "decoded rows are x, y, z, intensity, timestamp: ld >= 5; got %lld", (long long)ld);
  return lvx_decode(c, format, d_file, bytes, F, frame_pos, counts, timestamp_ns, point_period_ns, d_rows, ld, nullptr,
                    d_tags);
}

int mc_lvx_decode_batch(mc_ctx* c, int format, const void* d_file, int64_t bytes, int32_t F, const int64_t* frame_pos,
                        const int64_t* counts, const int64_t* timestamp_ns, int64_t point_period_ns, mc_batch* out,
                        uint8_t* d_tags) {
  CHECK_ARG(out, "batch is NULL");
  return lvx_decode(c, format, d_file, bytes, F, frame_pos, counts, timestamp_ns, point_period_ns, nullptr, 5, out,
                    d_tags);
}

int mc_text_lines(mc_ctx* c, const void* d_text, int64_t bytes, int64_t* n_lines) {
  CHECK_ARG(c, "ctx is NULL");
  DeviceGuard g(c->device);
  std::vector<int64_t> tile_off;
  return text_count(c, d_text, bytes, tile_off, n_lines);
}

int mc_text_decode(mc_ctx* c, int sep, int32_t n_cols, const void* d_text, int64_t bytes, int64_t n_lines,
                   double* d_rows, int64_t ld, int64_t* bad_line) {
  return text_decode(c, sep, n_cols, d_text, bytes, n_lines, d_rows, ld, nullptr, nullptr, nullptr, bad_line);
}

int mc_text_decode_batch(mc_ctx* c, int sep, int32_t n_cols, const void* d_text, int64_t bytes, mc_batch* out,
                         const int64_t* frame_start_ns, int64_t* frame_start_out, int64_t* bad_line) {
  CHECK_ARG(out, "batch is NULL");
  return text_decode(c, sep, n_cols, d_text, bytes, 0, nullptr, 0, out, frame_start_ns, frame_start_out, bad_line);
}

}  // extern "C"

// ---- LAS 1.2 (f8): save_las (LMC:950-963) / _export_las (CSIM:1671-1698) and their inverse ---------
namespace {

struct LasWrite {
  int fmt;
  const double* scale;
  const double* off;
  double imul, tmul;
  const char* software;
  int32_t year, doy;
};

int las_encode(mc_ctx* c, const Source& src, int64_t n, const LasWrite& p, void* d_out, int64_t out_bytes,
               int64_t* bad_row) {
  if (bad_row) *bad_row = -1;
  const int64_t reclen = mclas::nominal(p.fmt);
  CHECK_ARG(reclen, "point format %d: formats 0 to 3 are written", p.fmt);
  CHECK_ARG(p.scale && p.off, "scale / offset is NULL");
  for (int k = 0; k < 3; ++k)
    CHECK_ARG(std::isfinite(p.scale[k]) && p.scale[k] > 0.0 && std::isfinite(p.off[k]),
              "scale must be finite and > 0, offset finite (axis %d: %g, %g)", k, p.scale[k], p.off[k]);
  CHECK_ARG(std::isfinite(p.imul) && std::isfinite(p.tmul), "the intensity / time multipliers must be finite");
  CHECK_ARG(p.year >= 0 && p.year <= 65535 && p.doy >= 0 && p.doy <= 366, "creation date %d / day %d", p.year, p.doy);
  CHECK_ARG(n >= 0, "negative point count");
  CHECK_ARG(n < ((int64_t)1 << 32), "LAS 1.2 stores the point count as a u32: %lld points do not fit", (long long)n);
  const int64_t need = mclas::kHeader + n * reclen;
  if (out_bytes < need)
    return fail(MC_ERR_SPACE, "LAS output needs %lld bytes, buffer has %lld", (long long)need, (long long)out_bytes);
  CHECK_ARG(d_out, "d_out is NULL");
  CHECK_ARG(n == 0 || src.aos || src.batch, "points pointer is NULL");
  DeviceGuard g(c->device);
  struct Stats {
    unsigned long long bad[2];
    int32_t mm[6];
  } st = {{0ull, ~0ull}, {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN}};
  if (n > 0) {
    const int64_t tiles = (n + kLasTile - 1) / kLasTile;   // < 2^23
    char* d = nullptr;
    if (int r = codec_scratch(c, sizeof st + (size_t)tiles * 6 * sizeof(int32_t), &d)) return r;
    HIPCHK(hipMemcpyAsync(d, &st, sizeof st, hipMemcpyHostToDevice, c->stream));
    LasEncArgs a;
    a.rows = src.aos;
    a.ld = src.ld;
    a.cols = src.batch ? src.batch->d_cols : nullptr;
    a.C = src.batch ? src.batch->C : 0;
    a.doff = src.batch ? src.batch->d_doff : nullptr;
    a.poff = src.batch ? src.batch->d_poff : nullptr;
    a.fstart = src.batch ? src.batch->d_frame_start : nullptr;
    a.F = src.batch ? src.batch->F : 0;
    a.n = n;
    std::copy_n(p.scale, 3, a.scale);
    std::copy_n(p.off, 3, a.off);
    a.imul = p.imul;
    a.tmul = p.tmul;
    a.fmt = p.fmt;
    a.reclen = (int32_t)reclen;
    a.body = static_cast<char*>(d_out) + mclas::kHeader;
    a.bad = reinterpret_cast<unsigned long long*>(d);
    a.tile_mm = reinterpret_cast<int32_t*>(d + sizeof st);
    const dim3 grid((uint32_t)tiles), blk(kCodecBlock);
    const dim3 rgrid((uint32_t)std::min<int64_t>((tiles + kCodecBlock - 1) / kCodecBlock, kLasReduceGrid));
    {
      TimedRegion tr(c, &codec_of(c).ev, c->stream);
      if (src.batch) hipLaunchKernelGGL(k_las_encode<true>, grid, blk, 0, c->stream, a);
      else hipLaunchKernelGGL(k_las_encode<false>, grid, blk, 0, c->stream, a);
      hipLaunchKernelGGL(k_las_minmax, rgrid, blk, 0, c->stream, (const int32_t*)a.tile_mm, tiles,
                         reinterpret_cast<int32_t*>(d + offsetof(Stats, mm)));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&st, d, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (st.bad[0]) {
      if (bad_row) *bad_row = (int64_t)st.bad[1];
      return fail(MC_ERR_INVALID,
                  "row %lld (the first of %llu): a coordinate is not finite or rint((v - offset) / scale) is outside "
                  "int32, or the intensity is NaN or outside 0..65535",
                  (long long)st.bad[1], st.bad[0]);
    }
  }
  uint8_t hdr[mclas::kHeader];
  mclas::write_header(hdr, p.fmt, n, p.scale, p.off, st.mm, p.software ? p.software : "mcdeskew", p.year, p.doy);
  HIPCHK(hipMemcpyAsync(d_out, hdr, sizeof hdr, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MC_OK;
}

int las_decode(mc_ctx* c, const void* d_file, int64_t bytes, int fmt, int64_t reclen, int64_t offset, int64_t n,
               const double* scale, const double* off, double* d_rows, int64_t ld, mc_batch* out, double iscale,
               const int64_t* frame_start_ns, int64_t* frame_start_out, int64_t* bad_row) {
  if (bad_row) *bad_row = -1;
  CHECK_ARG(c && d_file && scale && off, "NULL argument");
  CHECK_ARG(((uintptr_t)d_file & 15) == 0, "d_file must be 16-byte aligned (and padded to a multiple of 16 bytes)");
  char msg[256];
  if (mclas::check_layout(bytes, fmt, reclen, offset, n, msg, sizeof msg)) return ingest_fail(msg);
  if (out) {
    CHECK_ARG(out->ctx == c, "batch belongs to another context");
    if (!out->has_t()) return fail(MC_ERR_STATE, "mc_las_decode_batch needs a batch created with MC_BATCH_WITH_TIME");
    CHECK_ARG(out->N == n, "the batch holds %lld points, the file %lld", (long long)out->N, (long long)n);
  } else {
    CHECK_ARG(n == 0 || d_rows, "d_rows is NULL");
  }
  DeviceGuard g(c->device);
  if (out && (frame_start_ns || n == 0)) {
    std::vector<int64_t> z((size_t)out->F, 0);
    const int64_t* s = frame_start_ns ? frame_start_ns : z.data();
    if (int r = mc_batch_set_frame_start_ns(out, s)) return r;
    if (frame_start_out) std::copy_n(s, out->F, frame_start_out);
  }
  if (n == 0) return MC_OK;
  unsigned long long bad[2] = {0ull, ~0ull};
  char* d = nullptr;
  if (int r = codec_scratch(c, sizeof bad, &d)) return r;
  HIPCHK(hipMemcpyAsync(d, bad, sizeof bad, hipMemcpyHostToDevice, c->stream));
  LasDecArgs a;
  a.file = static_cast<const uint8_t*>(d_file);
  a.offset = offset;
  a.fmt = fmt;
  a.reclen = (int32_t)reclen;
  a.n = n;
  std::copy_n(scale, 3, a.scale);
  std::copy_n(off, 3, a.off);
  a.rows = d_rows;
  a.ld = ld;
  a.cols = out ? out->d_cols : nullptr;
  a.doff = out ? out->d_doff : nullptr;
  a.poff = out ? out->d_poff : nullptr;
  a.fstart = out ? out->d_frame_start : nullptr;
  a.F = out ? out->F : 0;
  a.iscale = iscale;
  a.bad = reinterpret_cast<unsigned long long*>(d);
  const dim3 grid((uint32_t)((n + kLasDecTile - 1) / kLasDecTile)), blk(kLasDecTile);
  {
    TimedRegion tr(c, &codec_of(c).ev, c->stream);
    if (out && !frame_start_ns)
      hipLaunchKernelGGL(k_las_frame_start, dim3((out->F + kCodecBlock - 1) / kCodecBlock), dim3(kCodecBlock), 0,
                         c->stream, a);
    if (out) hipLaunchKernelGGL(k_las_decode<true>, grid, blk, 0, c->stream, a);
    else hipLaunchKernelGGL(k_las_decode<false>, grid, blk, 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  if (out) {
    HIPCHK(hipMemcpyAsync(bad, d, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    if (!frame_start_ns) {
      std::vector<int64_t> fs((size_t)out->F);
      HIPCHK(hipMemcpyAsync(fs.data(), out->d_frame_start, fs.size() * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      out->state.frame_starts_set();   // (the kernel wrote them)
      if (frame_start_out) std::copy(fs.begin(), fs.end(), frame_start_out);
    }
    if (int r = mcimpl::batch_columns_written(out, mcimpl::kWroteAllQueued)) return r;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (bad[0]) {
    if (bad_row) *bad_row = (int64_t)bad[1];
    return fail(MC_ERR_INVALID,
                "point %lld (the first of %llu): rint(gps_time * 1e9) minus its frame start does not fit int32 "
                "nanoseconds", (long long)bad[1], bad[0]);
  }
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_las_probe(const void* file, int64_t bytes, int32_t* point_format, int32_t* record_length,
                 int64_t* offset_to_points, int64_t* n_points, double* scale, double* offset, double* bounds) {
  char msg[256];
  mclas::Header h;
  if (mclas::probe(static_cast<const uint8_t*>(file), bytes, &h, msg, sizeof msg)) return ingest_fail(msg);
  if (point_format) *point_format = h.format;
  if (record_length) *record_length = h.reclen;
  if (offset_to_points) *offset_to_points = h.offset;
  if (n_points) *n_points = h.n;
  if (scale) std::copy_n(h.scale, 3, scale);
  if (offset) std::copy_n(h.off, 3, offset);
  if (bounds) std::copy_n(h.bounds, 6, bounds);
  return MC_OK;
}

int mc_las_encode(mc_ctx* c, const double* d_rows, int64_t ld, int64_t n, int point_format, const double* scale,
                  const double* offset, double intensity_mul, double time_mul, const char* software, int32_t year,
                  int32_t day_of_year, void* d_out, int64_t out_bytes, int64_t* bad_row) {
  CHECK_ARG(c, "ctx is NULL");
  const int64_t need = time_mul != 0.0 ? 5 : 4;
  if (ld < need)
    return fail(MC_ERR_INDEX, "LAS rows are x, y, z, intensity%s: ld >= %lld; got %lld", need == 5 ? ", timestamp" : "",
                (long long)need, (long long)ld);
  Source src;
  src.aos = d_rows;
  src.ld = ld;
  return las_encode(c, src, n, {point_format, scale, offset, intensity_mul, time_mul, software, year, day_of_year},
                    d_out, out_bytes, bad_row);
}

int mc_las_encode_batch(mc_ctx* c, const mc_batch* b, int point_format, const double* scale, const double* offset,
                        double intensity_mul, double time_mul, const char* software, int32_t year, int32_t day_of_year,
                        void* d_out, int64_t out_bytes, int64_t* bad_row) {
  CHECK_ARG(c && b, "NULL argument");
  CHECK_ARG(b->ctx == c, "batch belongs to another context");
  if (time_mul != 0.0) {
    if (!b->has_t()) return fail(MC_ERR_STATE, "a LAS time needs a batch created with MC_BATCH_WITH_TIME");
    if (!b->state.has_frame_starts()) return fail(MC_ERR_STATE, "the batch's frame starts are not set (mc_batch_set_frame_start_ns)");
  }
  Source src;
  src.batch = b;
  return las_encode(c, src, b->N, {point_format, scale, offset, intensity_mul, time_mul, software, year, day_of_year},
                    d_out, out_bytes, bad_row);
}

int mc_las_decode(mc_ctx* c, const void* d_file, int64_t bytes, int point_format, int64_t record_length,
                  int64_t offset_to_points, int64_t n_points, const double* scale, const double* offset, double* d_rows,
                  int64_t ld) {
  if (ld < 5) return fail(MC_ERR_INDEX, "decoded rows are x, y, z, intensity, gps_time: ld >= 5; got %lld", (long long)ld);
  return las_decode(c, d_file, bytes, point_format, record_length, offset_to_points, n_points, scale, offset, d_rows, ld,
                    nullptr, 1.0, nullptr, nullptr, nullptr);
}

int mc_las_decode_batch(mc_ctx* c, const void* d_file, int64_t bytes, int point_format, int64_t record_length,
                        int64_t offset_to_points, int64_t n_points, const double* scale, const double* offset,
                        double intensity_scale, mc_batch* out, const int64_t* frame_start_ns, int64_t* frame_start_out,
                        int64_t* bad_row) {
  CHECK_ARG(out, "batch is NULL");
  return las_decode(c, d_file, bytes, point_format, record_length, offset_to_points, n_points, scale, offset, nullptr, 5,
                    out, intensity_scale, frame_start_ns, frame_start_out, bad_row);
}

}  // extern "C"

extern "C" {

int mc_timing_read_codec(mc_ctx* c, double* ms, int64_t* n) {
  CHECK_ARG(c, "ctx is NULL");
  return read_timing(c, codec_of(c).ev, ms, n);
}

}  // extern "C"
