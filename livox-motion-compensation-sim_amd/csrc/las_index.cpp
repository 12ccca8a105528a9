// las_index.cpp — see las_index.hpp.  Every read is bounds-checked against `bytes` first.
#include "las_index.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace mclas {
namespace {

int bad(char* msg, size_t n, const char* fmt, ...) {
  if (msg && n) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, n, fmt, ap);
    va_end(ap);
  }
  return -1;
}

template <typename T>
T rd(const uint8_t* p) {   // little-endian hosts only, as the rest of the library
  T v;
  std::memcpy(&v, p, sizeof(T));
  return v;
}
template <typename T>
void wr(uint8_t* p, T v) {
  std::memcpy(p, &v, sizeof(T));
}

// X * scale + offset: the product rounded, then the sum (never one fused operation)
double bound(int32_t X, double scale, double off) {
  volatile double p = (double)X * scale;
  return p + off;
}

}  // namespace

int64_t nominal(int format) {
  return format == 0 ? 20 : format == 1 ? 28 : format == 2 ? 26 : format == 3 ? 34 : 0;
}

int check_layout(int64_t bytes, int format, int64_t reclen, int64_t offset, int64_t n, char* msg, size_t len) {
  const int64_t nom = nominal(format);
  if (!nom) return bad(msg, len, "point format %d: only formats 0..3 are decoded", format);
  if (reclen < nom || reclen > 65535)
    return bad(msg, len, "record length %lld: format %d needs %lld..65535 bytes", (long long)reclen, format,
               (long long)nom);
  if (offset < kHeader || offset > bytes)
    return bad(msg, len, "offset to point data %lld outside [227, %lld]", (long long)offset, (long long)bytes);
  if (n < 0 || n > 0xFFFFFFFFll) return bad(msg, len, "point count %lld outside 0..2^32-1", (long long)n);
  if (n > (bytes - offset) / reclen)   // n * reclen < 2^48: no overflow either way
    return bad(msg, len, "%lld records of %lld bytes from byte %lld run past the end (%lld bytes)", (long long)n,
               (long long)reclen, (long long)offset, (long long)bytes);
  return 0;
}

int probe(const uint8_t* file, int64_t bytes, Header* h, char* msg, size_t len) {
  if (!file || bytes <= 0) return bad(msg, len, "the file is empty");
  if (bytes < 4 || std::memcmp(file, "LASF", 4) != 0) return bad(msg, len, "unknown file signature (\"LASF\" expected)");
  if (bytes < kHeader)
    return bad(msg, len, "the file ends inside its 227-byte public header block (%lld bytes)", (long long)bytes);
  const int major = file[24], minor = file[25];
  if (major != 1 || minor > 3) return bad(msg, len, "LAS version %d.%d: versions 1.0 to 1.3 are decoded", major, minor);
  const int format = file[104];
  if (format > 3) return bad(msg, len, "point format %d: only formats 0..3 are decoded (no LAZ, no LAS 1.4 formats)", format);
  const int64_t header_size = rd<uint16_t>(file + 94);
  const int64_t offset = rd<uint32_t>(file + 96);
  if (header_size < kHeader) return bad(msg, len, "header size %lld below the 227 bytes of LAS 1.2", (long long)header_size);
  if (offset < header_size)
    return bad(msg, len, "offset to point data %lld lies inside the %lld-byte header", (long long)offset,
               (long long)header_size);
  const int64_t reclen = rd<uint16_t>(file + 105), n = rd<uint32_t>(file + 107);
  if (int r = check_layout(bytes, format, reclen, offset, n, msg, len)) return r;
  if (h) {
    h->format = format;
    h->reclen = (int32_t)reclen;
    h->offset = offset;
    h->n = n;
    for (int k = 0; k < 3; ++k) {
      h->scale[k] = rd<double>(file + 131 + 8 * k);
      h->off[k] = rd<double>(file + 155 + 8 * k);
    }
    for (int k = 0; k < 6; ++k) h->bounds[k] = rd<double>(file + 179 + 8 * k);
  }
  return 0;
}

void write_header(uint8_t out[kHeader], int format, int64_t n, const double scale[3], const double off[3],
                  const int32_t minmax[6], const char* software, int year, int day_of_year) {
  std::memset(out, 0, kHeader);
  std::memcpy(out, "LASF", 4);
  out[24] = 1;
  out[25] = 2;
  std::memcpy(out + 26, "OTHER", 5);
  if (software) std::memcpy(out + 58, software, strnlen(software, 32));
  wr<uint16_t>(out + 90, (uint16_t)day_of_year);
  wr<uint16_t>(out + 92, (uint16_t)year);
  wr<uint16_t>(out + 94, (uint16_t)kHeader);
  wr<uint32_t>(out + 96, (uint32_t)kHeader);
  out[104] = (uint8_t)format;
  wr<uint16_t>(out + 105, (uint16_t)nominal(format));
  wr<uint32_t>(out + 107, (uint32_t)n);
  for (int k = 0; k < 3; ++k) {
    wr<double>(out + 131 + 8 * k, scale[k]);
    wr<double>(out + 155 + 8 * k, off[k]);
    if (n > 0) {
      wr<double>(out + 179 + 16 * k, bound(minmax[2 * k + 1], scale[k], off[k]));   // max
      wr<double>(out + 187 + 16 * k, bound(minmax[2 * k], scale[k], off[k]));       // min
    }
  }
}

}  // namespace mclas
