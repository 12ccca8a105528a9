// ingest_index.hpp — the host walk over a recorded LVX file (f7, the inverse of f3 and f6): sniff the
// layout from the bytes, count and locate the frames, read the device info block and refuse whatever
// the decode kernels must not be launched on.  Plain C++ (no HIP include): the bytes are untrusted,
// so the walker is also linked into a stand-alone ASan / UBSan program by the tests.
//
//   MC_LVX_V11          LMC:57-272             "livox_tech", version 1.1.0.0, 88 header bytes; per frame
//                                              own offset, next offset (0 = last), frame id, then
//                                              1366-byte packages (22 B header, 96 x 14 B records)
//   MC_CSIM_LVX_LEGACY  CSIM:256-267, 295-321  "livox_file", 60 header bytes; per frame u64 timestamp,
//                                              u32 count, count x 14 B float32 records
//   MC_CSIM_LVX2        CSIM:269-293, 323-374  "livox_tech" + "2.0.0", 88 header bytes; per frame a 24 B
//                                              header and a 21 B package header, count x 14 B mm records
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mcingest {

constexpr int kFmtV11 = 0;          // = MC_LVX_V11
constexpr int kFmtCsimLegacy = 1;   // = MC_CSIM_LVX_LEGACY
constexpr int kFmtCsimLvx2 = 2;     // = MC_CSIM_LVX2 (lvx3 is the same bytes)

constexpr int64_t kRec = 14;
constexpr int64_t kV11FileHdr = 88, kV11FrameHdr = 24, kV11PkgHdr = 22, kV11PkgPoints = 96;
constexpr int64_t kV11Pkg = kV11PkgHdr + kV11PkgPoints * kRec;   // 1366
constexpr int64_t kLegacyFileHdr = 60, kLegacyFrameHdr = 12;
constexpr int64_t kLvx2FileHdr = 88, kLvx2FrameHdr = 45;
constexpr uint32_t kMagic = 0xAC0EA767u;

struct DeviceBlock {
  uint8_t sn[16];
  uint8_t device_type;
  uint8_t extrinsic_enable;
  float extrinsics[6];   // roll, pitch, yaw, x, y, z (zero where the layout stores none)
};

// file header bytes / frame header bytes of a format (0 for an unknown one)
int64_t file_header_bytes(int format);
int64_t frame_header_bytes(int format);

// 0, or -1 with a message in msg[0 .. msg_len).  *format, *n_frames: what the whole, validated walk found.
int probe(const uint8_t* file, int64_t bytes, int* format, int32_t* n_frames, char* msg, size_t msg_len);

// The same walk, filling frame_pos[F + 1] (each frame header's byte offset, then the file size),
// slots[F] (record slots: 96 x packages for V11, the stored count otherwise), frame_ids[F] (V11: the
// stored id; CSIM lvx2: the stored frame index; legacy: the position), timestamp_ns[F] (V11: the first
// package's timestamp, -1 for a frame without a package) and *dev.  Any output may be null.  format
// and n_frames must be what probe() reported for these bytes.
int index(const uint8_t* file, int64_t bytes, int format, int32_t n_frames, int64_t* frame_pos, int64_t* slots,
          uint64_t* frame_ids, int64_t* timestamp_ns, DeviceBlock* dev, char* msg, size_t msg_len);

// What a decode launch relies on, checked against the file size alone (the kernels never follow an
// offset stored in the file): frame_pos increasing from the file header to `bytes`, each frame's span
// a header plus whole packages (V11) or exactly counts[f] records (CSIM), 0 <= counts[f] <= slots.
// counts may be null for V11 (positions only).
int check_layout(int format, int64_t bytes, int32_t n_frames, const int64_t* frame_pos, const int64_t* counts,
                 char* msg, size_t msg_len);

}  // namespace mcingest
