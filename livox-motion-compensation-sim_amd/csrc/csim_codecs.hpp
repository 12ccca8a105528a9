// csim_codecs.hpp — gfx950 kernels for the output formats of livox_mid70_complete_simulator.py (CSIM):
//
//   LivoxLVXWriter.write_lvx_file   CSIM:235-374    lvx2 / lvx3 (int32 mm records behind one 45-byte
//                                                   frame + package header per frame) and legacy lvx
//                                                   (float32 records behind a 12-byte frame header)
//   DataExporter._export_pcd        CSIM:1643-1669  "%.6f %.6f %.6f %.0f %.0f\n"
//   DataExporter._export_xyz        CSIM:1700-1706  "%.6f %.6f %.6f\n" (np.savetxt)
//   DataExporter._export_csv        CSIM:1708-1715  "%.6f,%.6f,%.6f,%.6f,%.6f\n", NaN as an empty field
//
// Sources: a device (N, ld >= 5) float64 row buffer [x, y, z, intensity, timestamp] with frames back
// to back (the array of CSIM:1627), or a MC_BATCH_WITH_TIME batch whose point is *defined* as the row
// [x, y, z, trunc(intensity), frame_start_ns[f] + t_ns] with the float32 values widened exactly.
//
// The building blocks are those of codecs.hpp: units mapped to frames through a prefix
// (CodecFrames), the exact "%.6f" formatter (fmt6_prepare / fmt6_write), the tile scan (block_scan)
// and pieces assembled in LDS at the file's offset modulo 16 and stored with codec_store_piece
// (16-byte non-temporal stores).  Unlike LVX v1.1 the lvx2 frames start at odd byte offsets (88 + the
// prefix sum of 45 + 14 n), so the records are assembled with byte granularity.
#pragma once
#include "codecs.hpp"
#include "csim_text_core.hpp"

namespace mc {

constexpr int kCsimRec = 14;
constexpr int kCsimLvx2FileHdr = 24 + 64;      // file header + private header (CSIM:272-283, 323-341)
constexpr int kCsimLvx2FrameHdr = 24 + 21;     // frame header + package header (CSIM:348-363; the code writes 21)
constexpr int kCsimLvx1FileHdr = 28 + 32;      // file header + device block (CSIM:295-306)
constexpr int kCsimLvx1FrameHdr = 8 + 4;       // timestamp, point count (CSIM:314-315)
constexpr int kCsimUnitPoints = 768;           // one unit = up to this many consecutive records of one frame
constexpr int kCsimLvxChunks = (kCsimUnitPoints * kCsimRec + kCsimLvx2FrameHdr + 16) / 16 + 1;   // 16-byte LDS chunks
static_assert(kCsimLvxChunks * 16 >= 15 + kCsimLvx2FrameHdr + kCsimUnitPoints * kCsimRec, "a unit's piece fits");
static_assert(kCsimLvxChunks <= 3 * kCodecBlock, "codec_store_piece: three chunks per lane");

struct CsimSrc {
  CodecFrames fr;            // rows (aos, ld) or a batch's columns (cols, C = 5, poff)
  const int64_t* fstart;     // batch source: frame_start_ns[F]
  const uint8_t* tags;       // [N] dense tag bytes, or null = 0
};

// columns 0..NC-1 of dense row `row` (frame f) as float64
template <int NC>
__device__ __forceinline__ void csim_row(const CsimSrc& s, int32_t f, int64_t row, double* c) {
  if (s.fr.cols) {
    const float* q = s.fr.cols + bidx(s.fr.C, 0, s.fr.poff[f] + (row - s.fr.doff[f]));
    c[0] = q[0]; c[1] = q[kBlkPts]; c[2] = q[2 * kBlkPts];
    if constexpr (NC > 3) c[3] = trunc((double)q[3 * kBlkPts]);                              // int(), CSIM:1047
    if constexpr (NC > 4) c[4] = (double)(s.fstart[f] + (int64_t)__float_as_int(q[4 * kBlkPts]));
    return;
  }
  const double* q = s.fr.aos + row * s.fr.ld;
#pragma unroll
  for (int k = 0; k < NC; ++k) c[k] = q[k];
}

// ---- LVX ---------------------------------------------------------------------------------------
struct CsimLvxArgs {
  CsimSrc src;
  const int64_t* frame_pos;     // [F + 1] byte offset of each frame in the file, then the file size
  const uint64_t* ts_ns;        // [F] frame['timestamp']
  char* out;                    // file base
  int* err;                     // set to 1 where the reference's struct.pack / int() raises
};

// byte t of frame f's header.  VER 2 (CSIM:348-363): u32 frame index, u64 timestamp, u32 count, 8
// zero bytes | 5, 0, 1, 0 | u32 0 | 1, 2 | 3 zero bytes | u64 timestamp.  VER 1 (CSIM:314-315): u64
// timestamp, u32 count.
template <int VER>
__device__ __forceinline__ uint8_t csim_hdr_byte(int t, uint32_t f, uint64_t ts, uint32_t count) {
  if constexpr (VER == 1) return t < 8 ? (uint8_t)(ts >> (8 * t)) : (uint8_t)(count >> (8 * (t - 8)));
  if (t < 4) return (uint8_t)(f >> (8 * t));
  if (t < 12) return (uint8_t)(ts >> (8 * (t - 4)));
  if (t < 16) return (uint8_t)(count >> (8 * (t - 12)));
  if (t >= 37) return (uint8_t)(ts >> (8 * (t - 37)));
  return t == 24 ? 5 : t == 26 ? 1 : t == 32 ? 1 : t == 33 ? 2 : 0;
}

// One unit = up to 768 consecutive records of one frame = one contiguous byte range of the file; a
// frame's first unit also carries the frame's header.  Phase 1: a thread per record writes its 14
// bytes (three little-endian 32-bit words, intensity, tag) into LDS at the file's offset modulo 16,
// byte by byte — lvx2 pieces start at odd offsets.  Phase 2: codec_store_piece.
// VER 2: int(v * 1000), one float64 multiply then truncation toward zero, no clip (CSIM:368-372); a
// NaN / infinite coordinate or a product outside int32 fails the reference's write.  VER 1: float32
// round-to-nearest-even as struct.pack('<f') (CSIM:319); a finite coordinate that rounds to +-inf
// raises OverflowError there.  The intensity byte is trunc(intensity); NaN or outside 0..255 fails.
template <int VER>
__global__ __launch_bounds__(kCodecBlock) void k_csim_lvx(const CsimLvxArgs a) {
  constexpr int HDR = VER == 1 ? kCsimLvx1FrameHdr : kCsimLvx2FrameHdr;
  __shared__ uint4 s_buf[kCsimLvxChunks];
  uint8_t* const s8 = reinterpret_cast<uint8_t*>(s_buf);
  const int64_t u = blockIdx.x;   // grid = units exactly
  const int32_t f = codec_frame_of(a.src.fr, u);
  const int64_t k0 = (u - a.src.fr.unit_off[f]) * kCsimUnitPoints;   // the unit's first record in its frame
  const int64_t frow = a.src.fr.doff[f];
  const int64_t fcount = a.src.fr.doff[f + 1] - frow;
  const int n = (int)min_i64(fcount - k0, kCsimUnitPoints);
  const int hdr = k0 == 0 ? HDR : 0;
  const int64_t S = a.frame_pos[f] + (k0 == 0 ? 0 : HDR + k0 * kCsimRec);   // piece start in the file
  const int lo = (int)(S & 15);
  const int body = lo + hdr;

  for (int i = threadIdx.x; i < n; i += kCodecBlock) {
    const int64_t row = frow + k0 + i;
    double c[4];
    csim_row<4>(a.src, f, row, c);
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if constexpr (VER == 1) {
        const float g = (float)c[k];
        if (isinf(g) && !isinf(c[k])) *a.err = 1;
        w[k] = __float_as_uint(g);
      } else {
        double t = trunc(c[k] * 1000.0);
        if (!(t >= -2147483648.0 && t <= 2147483647.0)) { *a.err = 1; t = 0.0; }   // NaN fails the test too
        w[k] = (uint32_t)(int32_t)t;
      }
    }
    double it = trunc(c[3]);
    if (!(it >= 0.0 && it <= 255.0)) { *a.err = 1; it = 0.0; }
    uint8_t* r = s8 + body + i * kCsimRec;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[4 * k] = (uint8_t)w[k]; r[4 * k + 1] = (uint8_t)(w[k] >> 8);
      r[4 * k + 2] = (uint8_t)(w[k] >> 16); r[4 * k + 3] = (uint8_t)(w[k] >> 24);
    }
    r[12] = (uint8_t)(int)it;
    r[13] = a.src.tags ? a.src.tags[row] : (uint8_t)0;
  }
  if ((int)threadIdx.x < hdr)
    s8[lo + threadIdx.x] = csim_hdr_byte<VER>((int)threadIdx.x, (uint32_t)f, a.ts_ns[f], (uint32_t)fcount);
  __syncthreads();
  codec_store_piece<kCodecBlock, kCsimLvxChunks>(a.out + (S - lo), reinterpret_cast<const char*>(s_buf), lo,
                                                 body + n * kCsimRec);
}

// headers of the frames without points (they have no unit): a thread per frame
template <int VER>
__global__ __launch_bounds__(kCodecBlock) void k_csim_lvx_frames(const CsimLvxArgs a) {
  constexpr int HDR = VER == 1 ? kCsimLvx1FrameHdr : kCsimLvx2FrameHdr;
  const int32_t f = blockIdx.x * kCodecBlock + threadIdx.x;
  if (f >= a.src.fr.F || a.src.fr.doff[f + 1] != a.src.fr.doff[f]) return;
  char* o = a.out + a.frame_pos[f];
  const uint64_t ts = a.ts_ns[f];
  for (int t = 0; t < HDR; ++t) o[t] = (char)csim_hdr_byte<VER>(t, (uint32_t)f, ts, 0u);
}

struct CsimTextArgs {
  CsimSrc src;
  CsimLine line;
  int32_t* tile_bytes;          // measure: text bytes of each tile
  const int64_t* tile_pos;      // write: byte offset of each tile's text in `out`
  char* out;
  int* err;                     // 1: a value beyond the formatters' range
};

constexpr int kCsimTileText = kPcdBlock * 96;   // LDS text per tile: a CSV line of LiDAR values is ~75 bytes

template <int NC>
__device__ __forceinline__ void csim_tile_line(const CsimTextArgs& a, int64_t u, int32_t f, CsimText& L) {
  bool valid;
  const int64_t row = pcd_row(a.src.fr, u, f, valid);
  L.len = 0;
  if (valid) {
    double c[NC];
    csim_row<NC>(a.src, f, row, c);
    csim_line_prepare(a.line, c, L, a.err);
  }
}

// A tile = 256 consecutive lines of one frame, one workgroup: line lengths, block sum.
template <int NC>
__global__ __launch_bounds__(kPcdBlock) void k_csim_text_measure(const CsimTextArgs a) {
  __shared__ int s_wave[kPcdBlock / 64];
  const int64_t u = blockIdx.x;   // grid = tiles exactly
  CsimText L;
  csim_tile_line<NC>(a, u, codec_frame_of(a.src.fr, u), L);
  int total;
  block_scan(L.len, s_wave, total);
  if (threadIdx.x == 0) a.tile_bytes[u] = total;
}

// The tile's lines formatted byte by byte into LDS at the tile's file offset modulo 16, then
// codec_store_piece; a tile whose text is larger than the LDS buffer (extreme magnitudes only) is
// written line by line straight to HBM.
template <int NC>
__global__ __launch_bounds__(kPcdBlock) void k_csim_text_write(const CsimTextArgs a) {
  __shared__ int s_wave[kPcdBlock / 64];
  __shared__ uint4 s_text4[kCsimTileText / 16 + 1];
  char* const s_text = reinterpret_cast<char*>(s_text4);
  const int64_t u = blockIdx.x;   // grid = tiles exactly
  CsimText L;
  csim_tile_line<NC>(a, u, codec_frame_of(a.src.fr, u), L);
  int total;
  const int excl = block_scan(L.len, s_wave, total) - L.len;
  const int64_t G = a.tile_pos[u];
  const int shift = (int)(G & 15);
  if (total + shift <= kCsimTileText) {   // workgroup-uniform
    if (L.len) csim_line_emit(a.line, L, s_text + shift + excl);
    __syncthreads();
    codec_store_piece<kPcdBlock>(a.out + (G - shift), s_text, shift, shift + total);
  } else if (L.len) {
    csim_line_emit(a.line, L, a.out + G + excl);
  }
}

}  // namespace mc
