// ingest.hpp — gfx950 kernels for f7, the inverse of the output codecs (codecs.hpp, csim_codecs.hpp):
// recorded LVX files and ASCII PCD / XYZ / CSV text decoded into device float64 rows
// [x, y, z, intensity, timestamp_ns] (+ a tag byte per point), or into the float32 columns of a batch.
//
//   k_lvx_trim     LVX v1.1 stores no point count and pads a frame's last package with zero records
//                  (LMC:245-250): a wave per frame counts that package's trailing all-zero records
//   k_lvx_decode   a unit = up to 768 records of one frame (the encoders' unit): the unit's file bytes
//                  come in with 16-byte loads into LDS at the file offset modulo 16 (the mirror of
//                  codec_store_piece), the 14-byte records are picked out of LDS
//   k_text_count   non-empty lines starting in each 16 KiB tile; the host scans the tiles
//   k_text_starts  one int64 byte offset per line
//   k_text_parse   a lane per line, 256 lines per workgroup, their text staged in LDS when it fits
//
// No kernel follows an offset or a count stored in the file: the host walk (ingest_index.cpp)
// validates every frame position and count against the file size before a launch, and the loader
// pads the device copy of the file to a multiple of 16 bytes, so the aligned 16-byte loads stay inside
// the allocation.  None of these formats stores a per-point time: a point's timestamp is its frame's
// (v1.1: its package's) plus point_period_ns x (index in frame).
#pragma once
#include "codecs.hpp"
#include "csim_codecs.hpp"
#include "ingest_token_core.hpp"

namespace mc {

// ---- LVX -----------------------------------------------------------------------------------------
constexpr int kIngestUnit = 768;   // records per unit = kLvxUnitPoints = kCsimUnitPoints
constexpr int kIngestChunks = (15 + kLvxPkgPerWG * kLvxPkg + 15) / 16 + 1;
static_assert(kIngestUnit == kLvxUnitPoints && kIngestUnit % kLvxPkgPoints == 0, "a v1.1 unit is whole packages");
static_assert(kIngestChunks * 16 >= 15 + kLvxPkgPerWG * kLvxPkg && kLvxPkgPerWG * kLvxPkg >= kIngestUnit * 14,
              "a unit's piece fits");

struct LvxInArgs {
  CodecFrames fr;            // doff = dense prefix of the decoded counts, unit_off, F, n_units (+ poff: batch)
  const uint8_t* file;       // the file, padded to a multiple of 16 bytes
  const int64_t* frame_pos;  // [F + 1]
  const int64_t* ts_ns;      // [F] frame timestamps (CSIM formats; v1.1 reads its package headers)
  int64_t period;            // point_period_ns
  double* rows; int64_t ld;  // rows (N, ld >= 5), or
  float* cols;               // a batch's blocked columns (C = 5)
  uint8_t* tags;             // [N] or null
};

__device__ __forceinline__ uint32_t ingest_le32(const uint8_t* r) {
  return (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
}

// FMT: 0 = LVX v1.1 (int32 mm, reflectivity / 255), 1 = CSIM legacy (float32), 2 = CSIM lvx2 (int32 mm)
template <int FMT, bool TO_BATCH>
__global__ __launch_bounds__(kCodecBlock) void k_lvx_decode(const LvxInArgs a) {
  constexpr int HDR = FMT == 0 ? kLvxFrameHdr : FMT == 1 ? kCsimLvx1FrameHdr : kCsimLvx2FrameHdr;
  __shared__ uint4 s_buf[kIngestChunks];
  const uint8_t* const s8 = reinterpret_cast<const uint8_t*>(s_buf);
  const int64_t u = blockIdx.x;   // grid = units exactly
  const int32_t f = codec_frame_of(a.fr, u);
  const int64_t k0 = (u - a.fr.unit_off[f]) * kIngestUnit;   // the unit's first record in its frame
  const int64_t frow = a.fr.doff[f];
  const int n = (int)min_i64(a.fr.doff[f + 1] - frow - k0, kIngestUnit);
  int64_t S;   // the piece's first byte in the file
  int len;
  if constexpr (FMT == 0) {
    S = a.frame_pos[f] + HDR + (k0 / kLvxPkgPoints) * kLvxPkg;
    len = (n + kLvxPkgPoints - 1) / kLvxPkgPoints * kLvxPkg;
  } else {
    S = a.frame_pos[f] + HDR + k0 * kCsimRec;
    len = n * kCsimRec;
  }
  const int lo = (int)(S & 15);
  const uint4* const g = reinterpret_cast<const uint4*>(a.file + (S - lo));
  const int nch = (lo + len + 15) >> 4;   // <= kIngestChunks; ends inside the file's 16-byte padding
  for (int c = threadIdx.x; c < nch; c += kCodecBlock) s_buf[c] = g[c];
  __syncthreads();

  for (int i = threadIdx.x; i < n; i += kCodecBlock) {
    const uint8_t* r;
    int64_t ts;
    if constexpr (FMT == 0) {
      const int pk = i / kLvxPkgPoints, slot = i - pk * kLvxPkgPoints;
      const uint8_t* h = s8 + lo + pk * kLvxPkg;
      ts = (int64_t)((uint64_t)ingest_le32(h + 14) | ((uint64_t)ingest_le32(h + 18) << 32));   // LMC:237
      r = h + kLvxPkgHdr + slot * kLvxRec;
    } else {
      ts = a.ts_ns[f];
      r = s8 + lo + i * kCsimRec;
    }
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t w = ingest_le32(r + 4 * k);
      if constexpr (FMT == 1) c[k] = (double)__uint_as_float(w);
      else c[k] = (double)(int32_t)w / 1000.0;
    }
    const double it = FMT == 0 ? (double)r[12] / 255.0 : (double)r[12];
    const int64_t in_frame = k0 + i;
    const int64_t row = frow + in_frame;
    if constexpr (TO_BATCH) {
      float* q = a.cols + bidx(5, 0, a.fr.poff[f] + in_frame);
      q[0] = (float)c[0]; q[kBlkPts] = (float)c[1]; q[2 * kBlkPts] = (float)c[2]; q[3 * kBlkPts] = (float)it;
      q[4 * kBlkPts] = __int_as_float((int32_t)(in_frame * a.period));   // the host checked the range
    } else {
      double* o = a.rows + row * a.ld;
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = it;
      o[4] = (double)(ts + in_frame * a.period);
    }
    if (a.tags) a.tags[row] = r[13];
  }
}

// counts[f] = the record slots of frame f without the trailing all-zero records of its last package
__global__ __launch_bounds__(kCodecBlock) void k_lvx_trim(const uint8_t* file, const int64_t* frame_pos, int32_t F,
                                                          int64_t* counts) {
  const int32_t f = blockIdx.x * (kCodecBlock / 64) + (int)(threadIdx.x >> 6);
  if (f >= F) return;   // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t end = frame_pos[f + 1];
  const int64_t pk = (end - frame_pos[f] - kLvxFrameHdr) / kLvxPkg;
  int64_t count = 0;
  if (pk > 0) {
    const uint8_t* rec = file + (end - kLvxPkg + kLvxPkgHdr);
    uint32_t o0 = 0, o1 = 0;
    for (int b = 0; b < kLvxRec; ++b) {
      o0 |= rec[lane * kLvxRec + b];
      if (lane < kLvxPkgPoints - 64) o1 |= rec[(64 + lane) * kLvxRec + b];
    }
    const uint64_t m0 = __builtin_amdgcn_ballot_w64(o0 != 0), m1 = __builtin_amdgcn_ballot_w64(o1 != 0);
    const int last = m1 ? 64 + 63 - __builtin_clzll(m1) : m0 ? 63 - __builtin_clzll(m0) : -1;
    count = (pk - 1) * kLvxPkgPoints + last + 1;
  }
  if (lane == 0) counts[f] = count;
}

// ---- text ----------------------------------------------------------------------------------------
constexpr int kTextLaneChunks = 4;                 // count / starts: consecutive 16-byte chunks per lane
constexpr int kTextTile = kPcdBlock * 16 * kTextLaneChunks;   // bytes per count / starts workgroup (16 KiB)
constexpr int kTextLines = kPcdBlock;              // lines per parse workgroup
constexpr int kTextLds = kPcdBlock * 96;           // parse: LDS text per tile (a CSV line is ~75 bytes)

// bit k: byte k of x equals the byte repeated in pat.  t = x ^ pat has a zero byte exactly there;
// (t & 0x7f..) + 0x7f.. carries into bit 7 of every byte with a low bit set and never across bytes, so
// ~(that | t | 0x7f..) leaves 0x80 in exactly the zero bytes; the multiply gathers the four flags.
__device__ __forceinline__ uint32_t text_eq4(uint32_t x, uint32_t pat) {
  const uint32_t t = x ^ pat;
  const uint32_t z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu);
  return (((z >> 7) * 0x00204081u) >> 21) & 0xfu;
}
__device__ __forceinline__ uint32_t text_eq16(const uint4& w, uint32_t pat) {
  return text_eq4(w.x, pat) | (text_eq4(w.y, pat) << 4) | (text_eq4(w.z, pat) << 8) | (text_eq4(w.w, pat) << 12);
}

// bit j: a non-empty line starts at byte b0 + j of the text, for the 16-byte chunk w at b0.  A line
// starts after a '\n' (or at byte 0); it is empty when it holds nothing or a lone '\r'.  prev_nl: the
// byte before the chunk is a '\n' (or the chunk is the first); after_end: the byte after the chunk is a
// '\n' or past the end.
__device__ __forceinline__ uint32_t text_mask16(const uint4& w, int64_t b0, int64_t bytes, bool prev_nl, bool after_end) {
  if (b0 >= bytes) return 0u;
  const uint32_t in = b0 + 16 <= bytes ? 0xffffu : (1u << (int)(bytes - b0)) - 1u;   // bytes of the chunk inside the text
  const uint32_t nl = text_eq16(w, 0x0a0a0a0au), cr = text_eq16(w, 0x0d0d0d0du);
  const uint32_t after_nl = ((nl << 1) | (prev_nl ? 1u : 0u)) & 0xffffu;                  // the byte before is a '\n'
  const uint32_t next_end = (((nl | ~in) & 0xffffu) >> 1) | (after_end ? 0x8000u : 0u);   // the byte after is a '\n' or the end
  return in & after_nl & ~nl & ~(cr & next_end);
}

// The kTextLaneChunks consecutive chunks of a lane, from chunk0 on: every load is issued before the
// first mask is formed (a chunk past the end re-reads the text's last chunk instead of branching, so
// the loads do not wait on one another), then the masks; only the two bytes outside the lane's 64 come
// from loads of their own.  bytes > 0.
__device__ __forceinline__ void text_lane_masks(const char* text, int64_t bytes, int64_t chunk0, uint32_t m[kTextLaneChunks]) {
  const int64_t last = (bytes - 1) >> 4;
  uint4 w[kTextLaneChunks];
#pragma unroll
  for (int j = 0; j < kTextLaneChunks; ++j)
    w[j] = *reinterpret_cast<const uint4*>(text + 16 * min_i64(chunk0 + j, last));   // inside the 16-byte padding
  const int64_t b0 = chunk0 * 16, bend = b0 + 16 * kTextLaneChunks;
  const bool prev_nl = b0 == 0 || b0 > bytes || text[b0 - 1] == '\n';
  const bool after_end = bend >= bytes || text[bend] == '\n';
#pragma unroll
  for (int j = 0; j < kTextLaneChunks; ++j) {
    // chunk j inside the text: chunk j - 1 is whole, and chunk j + 1 is its own data unless the text ends first
    const bool p = j == 0 ? prev_nl : (w[j > 0 ? j - 1 : 0].w >> 24) == (uint32_t)'\n';
    const bool e = j == kTextLaneChunks - 1 ? after_end
                                            : (b0 + 16 * (j + 1) >= bytes || (w[j + 1 < kTextLaneChunks ? j + 1 : j].x & 0xffu) == (uint32_t)'\n');
    m[j] = text_mask16(w[j], b0 + 16 * j, bytes, p, e);
  }
}

__global__ __launch_bounds__(kPcdBlock) void k_text_count(const char* text, int64_t bytes, int32_t* tile_count) {
  __shared__ int s_wave[kPcdBlock / 64];
  uint32_t m[kTextLaneChunks];
  text_lane_masks(text, bytes, ((int64_t)blockIdx.x * kPcdBlock + threadIdx.x) * kTextLaneChunks, m);
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kTextLaneChunks; ++j) cnt += __popc(m[j]);
  int total;
  block_scan(cnt, s_wave, total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// starts[tile_off[tile] + ...] = the byte offset of each line starting in the tile
__global__ __launch_bounds__(kPcdBlock) void k_text_starts(const char* text, int64_t bytes, const int64_t* tile_off,
                                                           int64_t* starts) {
  __shared__ int s_wave[kPcdBlock / 64];
  const int64_t chunk0 = ((int64_t)blockIdx.x * kPcdBlock + threadIdx.x) * kTextLaneChunks;
  uint32_t m[kTextLaneChunks];
  text_lane_masks(text, bytes, chunk0, m);
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kTextLaneChunks; ++j) cnt += __popc(m[j]);
  int total;
  int64_t at = tile_off[blockIdx.x] + (block_scan(cnt, s_wave, total) - cnt);
#pragma unroll
  for (int j = 0; j < kTextLaneChunks; ++j) {
    uint32_t w = m[j];
    while (w) {
      const int b = __builtin_ctz(w);
      w &= w - 1;
      starts[at++] = (chunk0 + j) * 16 + b;
    }
  }
}

struct TextArgs {
  const char* text;
  int64_t bytes;
  const int64_t* starts;      // [n_lines + 1], the last = bytes
  int64_t n_lines;
  int32_t n_cols;
  int32_t sep;
  double* rows; int64_t ld;   // rows (n_lines, ld >= n_cols), or
  float* cols; int32_t C;     // a batch's blocked columns
  const int64_t* doff;        // batch: [F + 1] dense line prefix of the frames
  const int64_t* poff;        // batch: [F + 1] padded offsets
  int32_t F;
  int64_t* fstart;            // batch with a time column: frame_start_ns[F]
  uint32_t* tile_flag;        // per parse tile: min over its faulty lines of (line in tile << 2 | kind), or ~0
};

__device__ __forceinline__ bool text_i64(double v, int64_t& out) {
  if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) return false;   // also NaN
  out = (int64_t)v;
  return true;
}

// default frame starts: each frame's first point's timestamp (column 4), 0 for an empty frame or a
// line the parse kernel will flag
__global__ __launch_bounds__(kPcdBlock) void k_text_frame_start(const TextArgs a) {
  const int32_t f = blockIdx.x * kPcdBlock + threadIdx.x;
  if (f >= a.F) return;
  int64_t s = 0;
  const int64_t l = a.doff[f];
  if (a.doff[f + 1] > l) {
    double v[kIngestMaxCols];
    if (ingest_line(a.text + a.starts[l], a.text + a.bytes, (char)a.sep, a.n_cols, a.sep == ',', v) == 0) {
      int64_t t;
      if (text_i64(v[4], t)) s = t;
    }
  }
  a.fstart[f] = s;
}

template <bool TO_BATCH>
__global__ __launch_bounds__(kPcdBlock) void k_text_parse(const TextArgs a) {
  __shared__ uint4 s_text4[kTextLds / 16 + 2];
  __shared__ uint32_t s_bad;
  const int64_t l0 = (int64_t)blockIdx.x * kTextLines;
  const int64_t l1 = min_i64(l0 + kTextLines, a.n_lines);
  const int64_t G0 = a.starts[l0], G1 = a.starts[l1];
  const int shift = (int)(G0 & 15);
  const bool staged = G1 - G0 + shift <= kTextLds;   // workgroup-uniform
  if (threadIdx.x == 0) s_bad = 0xffffffffu;
  if (staged) {
    const uint4* g = reinterpret_cast<const uint4*>(a.text + (G0 - shift));
    const int nch = (int)((G1 - G0 + shift + 15) >> 4);   // ends inside the text's 16-byte padding
    for (int c = threadIdx.x; c < nch; c += kPcdBlock) s_text4[c] = g[c];
  }
  __syncthreads();
  const int64_t l = l0 + threadIdx.x;
  if (l < l1) {
    double v[kIngestMaxCols];
    const int64_t at = a.starts[l] - G0, end = G1 - G0;
    int bad;
    if (staged) {   // two calls: the staged one reads LDS with ds loads, not through a generic pointer
      const char* base = reinterpret_cast<const char*>(s_text4) + shift;
      bad = ingest_line(base + at, base + end, (char)a.sep, a.n_cols, a.sep == ',', v);
    } else {
      const char* base = a.text + G0;
      bad = ingest_line(base + at, base + end, (char)a.sep, a.n_cols, a.sep == ',', v);
    }
    if (!bad) {
      if constexpr (TO_BATCH) {
        int32_t lo = 0, hi = a.F + 1;   // frame of line l: the last f with doff[f] <= l
        while (lo < hi) {
          const int32_t mid = (lo + hi) >> 1;
          if (a.doff[mid] <= l) lo = mid + 1; else hi = mid;
        }
        const int32_t f = lo - 1;
        float* q = a.cols + bidx(a.C, 0, a.poff[f] + (l - a.doff[f]));
        q[0] = (float)v[0]; q[kBlkPts] = (float)v[1]; q[2 * kBlkPts] = (float)v[2];
        q[3 * kBlkPts] = a.n_cols > 3 ? (float)v[3] : 0.0f;
        if (a.C == 5) {
          int64_t t = 0;
          if (a.n_cols > 4) {
            int64_t ti;
            const bool fits = text_i64(v[4], ti);
            const __int128 d = fits ? (__int128)ti - (__int128)a.fstart[f] : (__int128)0;
            if (!fits || d < -2147483648ll || d > 2147483647ll) bad = kIngestBadTime; else t = (int64_t)d;
          }
          q[4 * kBlkPts] = __int_as_float((int32_t)t);
        }
      } else {
        double* o = a.rows + l * a.ld;
#pragma unroll
        for (int k = 0; k < kIngestMaxCols; ++k) {
          if (k >= a.n_cols) break;
          o[k] = v[k];
        }
      }
    }
    if (bad) atomicMin(&s_bad, ((uint32_t)threadIdx.x << 2) | (uint32_t)bad);
  }
  __syncthreads();
  if (threadIdx.x == 0) a.tile_flag[blockIdx.x] = s_bad;
}

}  // namespace mc
