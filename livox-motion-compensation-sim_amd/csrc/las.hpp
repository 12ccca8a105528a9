// las.hpp — gfx950 kernels for f8, the LAS 1.2 codec (LMC:950-963 save_las, CSIM:1671-1698
// _export_las; both are thin laspy calls in the reference): point formats 0..3 written from device
// float64 rows or a batch's float32 columns, and read back into rows or a batch.
//
//   k_las_encode   a tile = kLasTile records of the dense body.  The body starts at file byte 227 and a
//                  record is 20 / 28 / 26 / 34 bytes, so no record is aligned; 8 records of any format
//                  are a multiple of 16 bytes, so every tile sits at the same offset modulo 16.  Records
//                  are OR-ed into a zeroed LDS image of the tile as shifted 32-bit words and leave with
//                  codec_store_piece: 16-byte stores, byte stores for the two ragged end chunks (no
//                  output byte is written by two workgroups).  Min / max of X, Y, Z reduced over each
//                  wave by DPP and over the tile in LDS, and the refused rows (count, first row), go to
//                  a second output with one atomic per value and tile.
//   k_las_decode   a tile = kLasDecTile records, a thread per record; the tile's file bytes come in with
//                  aligned 16-byte loads into LDS (as k_lvx_decode) when they fit, else the records are
//                  read in place (record lengths far above the nominal size).
//
// No kernel follows a number stored in the file: the host (las_index.cpp) validates offset, record
// length and count against the file size before a launch, and the loader pads the device copy of the
// file to a multiple of 16 bytes.
#pragma once
#include "codecs.hpp"
#include "las_core.hpp"

namespace mc {

constexpr int kLasTile = 512;       // records per encode workgroup; a multiple of 8 (8 x reclen % 16 == 0)
constexpr int kLasMaxRec = 34;
constexpr int kLasEncChunks = (15 + kLasTile * kLasMaxRec + 15) / 16;
constexpr int kLasDecTile = 256;    // records per decode workgroup
constexpr int kLasDecLds = kLasDecTile * 48;   // a tile is staged in LDS when offset % 16 + its bytes fit
constexpr int kLasDecChunks = (kLasDecLds + 15) / 16 + 1;
static_assert(kLasTile % 8 == 0 && kLasTile % kCodecBlock == 0, "tiles share one phase; whole passes of the workgroup");

typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ void lds_or32(uint32_t* p, uint32_t v) {
  __hip_atomic_fetch_or((lds_u32*)(void*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// K little-endian words at byte b of the zeroed LDS image: shifted onto the 4-byte grid, K (+ 1 when
// b % 4 != 0) ds_or_b32; the zero bytes of a shifted word leave the neighbouring records alone
template <int K>
__device__ __forceinline__ void las_or_words(uint32_t* s32, int b, const uint32_t (&w)[K]) {
  const int s = 8 * (b & 3);
  uint32_t* const p = s32 + (b >> 2);
  uint32_t prev = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    lds_or32(p + j, (uint32_t)((((uint64_t)w[j] << 32) | prev) >> (32 - s)));
    prev = w[j];
  }
  if (s) lds_or32(p + K, prev >> (32 - s));   // starts below b + 4 K: inside the record
}

// the wave's minimum / maximum in every lane: DPP inside each 16-lane row (pairs, quads, half-row and
// row mirrors; a lane without a source keeps its own value), then the four rows from lanes 0, 16, 32,
// 48.  Every lane of the wave must be active.
template <bool MAX>
__device__ __forceinline__ int las_wave_minmax(int v) {
  const auto pick = [](int a, int b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); };
  v = pick(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
  v = pick(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
  v = pick(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = pick(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
  return pick(pick(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
              pick(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

struct LasEncArgs {
  const double* rows; int64_t ld;   // rows (n, ld >= 4; >= 5 when tmul != 0), or
  const float* cols; int32_t C;     // a batch's blocked columns
  const int64_t* doff;              // batch: [F + 1] dense prefix of the frames
  const int64_t* poff;              // batch: [F + 1] padded offsets
  const int64_t* fstart;            // batch with time: frame_start_ns[F]
  int32_t F;
  int64_t n;
  double scale[3], off[3];
  double imul, tmul;
  int32_t fmt, reclen;
  char* body;                       // the first record's byte (file base + 227)
  int32_t* tile_mm;                 // [tiles][6] min X, max X, min Y, max Y, min Z, max Z of each tile's accepted rows
  unsigned long long* bad;          // [2] refused rows, the first of them (start: 0, ~0)
};

// the frame holding dense row `row` (row < doff[F]): the last f with doff[f] <= row
__device__ __forceinline__ int32_t las_frame_of(const int64_t* doff, int32_t F, int64_t row) {
  int32_t lo = 0, hi = F;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (doff[mid] <= row) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

template <bool FROM_BATCH>
__global__ __launch_bounds__(kCodecBlock) void k_las_encode(const LasEncArgs a) {
  __shared__ uint4 s_buf[kLasEncChunks];
  __shared__ int s_mm[kCodecBlock / 64][6];
  __shared__ unsigned s_nbad, s_first;
  uint32_t* const s32 = reinterpret_cast<uint32_t*>(s_buf);
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kLasTile;   // grid = tiles exactly
  const int cnt = (int)min_i64(a.n - r0, kLasTile);
  const int phase = (int)(reinterpret_cast<uintptr_t>(a.body) & 15);   // of every tile: kLasTile * reclen % 16 == 0
  const int bytes = cnt * a.reclen;
  const int nch = (phase + bytes + 15) >> 4;   // <= kLasEncChunks
  for (int c = tid; c < nch; c += kCodecBlock) s_buf[c] = make_uint4(0u, 0u, 0u, 0u);
  if (tid == 6) s_nbad = 0u;
  if (tid == 7) s_first = 0xffffffffu;
  __syncthreads();

  int32_t f = 0;
  if constexpr (FROM_BATCH) f = las_frame_of(a.doff, a.F, r0);
  int mm[6] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};   // this lane's records
#pragma unroll
  for (int j = 0; j < kLasTile / kCodecBlock; ++j) {
    const int i = j * kCodecBlock + tid;
    if (i >= cnt) break;
    const int64_t row = r0 + i;
    double c[5];
    if constexpr (FROM_BATCH) {
      while (a.doff[f + 1] <= row) ++f;   // row < doff[F]
      const float* q = a.cols + bidx(a.C, 0, a.poff[f] + (row - a.doff[f]));
      c[0] = q[0]; c[1] = q[kBlkPts]; c[2] = q[2 * kBlkPts]; c[3] = q[3 * kBlkPts];
      c[4] = a.tmul != 0.0 ? (double)(a.fstart[f] + (int64_t)__float_as_int(q[4 * kBlkPts])) : 0.0;   // C == 5: host-checked
    } else {
      const double* q = a.rows + row * a.ld;
      c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; c[3] = q[3];
      c[4] = a.tmul != 0.0 ? q[4] : 0.0;   // ld >= 5: host-checked
    }
    const LasRec r = las_encode_rec(c, a.scale, a.off, a.imul, a.tmul);
    if (r.bad) {
      atomicAdd(&s_nbad, 1u);
      atomicMin(&s_first, (unsigned)i);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        mm[2 * k] = r.X[k] < mm[2 * k] ? r.X[k] : mm[2 * k];
        mm[2 * k + 1] = r.X[k] > mm[2 * k + 1] ? r.X[k] : mm[2 * k + 1];
      }
    }
    const int b = phase + i * a.reclen;
    const uint32_t w[4] = {(uint32_t)r.X[0], (uint32_t)r.X[1], (uint32_t)r.X[2], r.intensity};
    las_or_words(s32, b, w);   // bytes 14..19 (flags, classification, angle, user data, source id) stay 0
    if (a.fmt & 1) {
      const uint64_t g = (uint64_t)__double_as_longlong(r.gps);
      const uint32_t t[2] = {(uint32_t)g, (uint32_t)(g >> 32)};
      las_or_words(s32, b + 20, t);   // formats 2, 3: R, G, B stay 0
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // every lane is back here
    const int lo = las_wave_minmax<false>(mm[2 * k]), hi = las_wave_minmax<true>(mm[2 * k + 1]);
    if ((tid & 63) == 0) { s_mm[tid >> 6][2 * k] = lo; s_mm[tid >> 6][2 * k + 1] = hi; }
  }
  __syncthreads();
  codec_store_piece<kCodecBlock, kLasEncChunks>(a.body + (r0 * a.reclen - phase), reinterpret_cast<const char*>(s_buf),
                                                phase, phase + bytes);
  if (tid < 6) {
    int v = s_mm[0][tid];
#pragma unroll
    for (int w = 1; w < kCodecBlock / 64; ++w) v = (tid & 1) ? (s_mm[w][tid] > v ? s_mm[w][tid] : v) : (s_mm[w][tid] < v ? s_mm[w][tid] : v);
    // per tile, reduced by k_las_minmax: one global atomic per tile on six words of one cache line
    // serialised the launch — 2699.3 vs 590.3 us from a batch, 2720.5 vs 836.4 us from rows, 60 M points
    // in 117 k tiles (profiles/las/bench.json, ab_minmax_atomics.txt)
    a.tile_mm[(int64_t)blockIdx.x * 6 + tid] = v;
  }
  if (tid == 6 && s_nbad) {
    atomicAdd(a.bad, (unsigned long long)s_nbad);
    atomicMin(a.bad + 1, (unsigned long long)(r0 + s_first));
  }
}

// mm[6] (start: INT32_MAX / INT32_MIN alternating) = min / max over the tiles' six values: a few
// workgroups stride over the tiles, a wave reduction, one atomic per wave and value
constexpr int kLasReduceGrid = 64;
__global__ __launch_bounds__(kCodecBlock) void k_las_minmax(const int32_t* tile_mm, int64_t tiles, int32_t* mm) {
  int v[6] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
  for (int64_t t = (int64_t)blockIdx.x * kCodecBlock + threadIdx.x; t < tiles; t += (int64_t)gridDim.x * kCodecBlock) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int x = tile_mm[t * 6 + k];
      v[k] = (k & 1) ? (x > v[k] ? x : v[k]) : (x < v[k] ? x : v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int r = (k & 1) ? las_wave_minmax<true>(v[k]) : las_wave_minmax<false>(v[k]);
    if ((threadIdx.x & 63) == 0) {
      if (k & 1) atomicMax(mm + k, r); else atomicMin(mm + k, r);
    }
  }
}

struct LasDecArgs {
  const uint8_t* file;              // the file, padded to a multiple of 16 bytes
  int64_t offset;                   // offset to point data
  int32_t fmt, reclen;
  int64_t n;
  double scale[3], off[3];
  double* rows; int64_t ld;         // rows (n, ld >= 5), or
  float* cols;                      // a batch's blocked columns (C = 5)
  const int64_t* doff;              // batch: [F + 1]
  const int64_t* poff;              // batch: [F + 1]
  int64_t* fstart;                  // batch: frame_start_ns[F]
  int32_t F;
  double iscale;                    // batch: intensity column = float32(intensity * iscale)
  unsigned long long* bad;          // batch: [2] points whose t_ns does not fit int32, the first of them
};

// default frame starts: each frame's first point's time in ns, 0 for an empty frame, a format without
// time or a time the decode kernel will flag
__global__ __launch_bounds__(kCodecBlock) void k_las_frame_start(const LasDecArgs a) {
  const int32_t f = blockIdx.x * kCodecBlock + threadIdx.x;
  if (f >= a.F) return;
  int64_t s = 0;
  const int64_t row = a.doff[f];
  if (a.doff[f + 1] > row && (a.fmt & 1)) {
    double v[5];
    las_decode_rec(a.file + (a.offset + row * a.reclen), a.fmt, a.scale, a.off, v);
    int64_t t;
    if (las_time_ns(v[4], &t)) s = t;
  }
  a.fstart[f] = s;
}

template <bool TO_BATCH>
__global__ __launch_bounds__(kLasDecTile) void k_las_decode(const LasDecArgs a) {
  __shared__ uint4 s_buf[kLasDecChunks];
  __shared__ unsigned s_nbad, s_first;
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kLasDecTile;   // grid = tiles exactly
  const int cnt = (int)min_i64(a.n - r0, kLasDecTile);
  const int64_t S = a.offset + r0 * a.reclen;   // the tile's first byte in the file
  const int lo = (int)(S & 15);
  const int len = cnt * a.reclen;               // <= 256 * 65535
  const bool staged = lo + len <= kLasDecLds;   // workgroup-uniform
  if (TO_BATCH && tid == 0) { s_nbad = 0u; s_first = 0xffffffffu; }
  if (staged) {
    const uint4* g = reinterpret_cast<const uint4*>(a.file + (S - lo));
    const int nch = (lo + len + 15) >> 4;       // <= kLasDecChunks; ends inside the file's 16-byte padding
    for (int c = tid; c < nch; c += kLasDecTile) s_buf[c] = g[c];
  }
  __syncthreads();
  if (tid < cnt) {
    double v[5];
    if (staged) las_decode_rec(reinterpret_cast<const uint8_t*>(s_buf) + lo + tid * a.reclen, a.fmt, a.scale, a.off, v);
    else las_decode_rec(a.file + (S + (int64_t)tid * a.reclen), a.fmt, a.scale, a.off, v);
    const int64_t row = r0 + tid;
    if constexpr (TO_BATCH) {
      int32_t f = las_frame_of(a.doff, a.F, r0);   // workgroup-uniform, then a step per frame boundary in the tile
      while (a.doff[f + 1] <= row) ++f;            // row < doff[F]
      float* q = a.cols + bidx(5, 0, a.poff[f] + (row - a.doff[f]));
      q[0] = (float)v[0]; q[kBlkPts] = (float)v[1]; q[2 * kBlkPts] = (float)v[2];
      q[3 * kBlkPts] = (float)(v[3] * a.iscale);
      int64_t t = 0;
      const bool fits = las_time_ns(v[4], &t);
      const __int128 d = fits ? (__int128)t - (__int128)a.fstart[f] : (__int128)0;
      const bool ok = fits && d >= -2147483648ll && d <= 2147483647ll;
      q[4 * kBlkPts] = __int_as_float(ok ? (int32_t)d : 0);
      if (!ok) {
        atomicAdd(&s_nbad, 1u);
        atomicMin(&s_first, (unsigned)tid);
      }
    } else {
      double* o = a.rows + row * a.ld;
      o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; o[4] = v[4];
    }
  }
  if constexpr (TO_BATCH) {
    __syncthreads();
    if (tid == 0 && s_nbad) {
      atomicAdd(a.bad, (unsigned long long)s_nbad);
      atomicMin(a.bad + 1, (unsigned long long)(r0 + s_first));
    }
  }
}

}  // namespace mc
