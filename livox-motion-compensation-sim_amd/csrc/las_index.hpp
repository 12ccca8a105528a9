// las_index.hpp — the host side of the LAS 1.2 codec (f8) that touches no device: the parser of an
// untrusted public header block and the writer of the 227-byte block the encoder puts ahead of its
// records.  Plain C++ (no HIP include): the parser reads untrusted bytes, so it is also linked into a
// stand-alone ASan / UBSan program by the tests.
//
// ASPRS LAS 1.2, little-endian.  Public header block (227 bytes): "LASF", source id u16 @4, global
// encoding u16 @6, GUID @8, version bytes @24, system identifier char[32] @26, generating software
// char[32] @58, creation day of year u16 @90, year u16 @92, header size u16 @94, offset to point data
// u32 @96, VLR count u32 @100, point format u8 @104, record length u16 @105, point count u32 @107,
// points by return u32[5] @111, scale xyz f64[3] @131, offset xyz f64[3] @155, then max x, min x,
// max y, min y, max z, min z f64 @179.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mclas {

constexpr int64_t kHeader = 227;

struct Header {
  int32_t format;      // 0..3
  int32_t reclen;      // >= nominal(format)
  int64_t offset;      // offset to point data, >= header size >= 227
  int64_t n;           // point count
  double scale[3], off[3];
  double bounds[6];    // max x, min x, max y, min y, max z, min z, as stored
};

// record bytes of point formats 0..3 (20, 28, 26, 34); 0 for any other
int64_t nominal(int format);

// 0 and *h, or -1 with a message in msg[0 .. msg_len).  Accepted: "LASF", version 1.0 .. 1.3, formats
// 0..3, header size >= 227, offset >= header size, record length >= nominal, offset + n * record length
// <= bytes.  Nothing is written to *h for a refused file.
int probe(const uint8_t* file, int64_t bytes, Header* h, char* msg, size_t msg_len);

// What a decode launch relies on, from the caller's numbers and the file size alone.
int check_layout(int64_t bytes, int format, int64_t reclen, int64_t offset, int64_t n, char* msg, size_t msg_len);

// The header of a file of n records without VLRs.  minmax: min X, max X, min Y, max Y, min Z, max Z
// of the stored integers (ignored when n == 0: the bounds are then 0.0); each bound is X * scale +
// offset in float64, a multiply then an add.  software: at most 32 bytes are used.
void write_header(uint8_t out[kHeader], int format, int64_t n, const double scale[3], const double off[3],
                  const int32_t minmax[6], const char* software, int year, int day_of_year);

}  // namespace mclas
