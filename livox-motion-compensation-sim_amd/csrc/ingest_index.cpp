// ingest_index.cpp — see ingest_index.hpp.  Every read is bounds-checked against `bytes` first.
#include "ingest_index.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace mcingest {
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

int sniff(const uint8_t* file, int64_t bytes, int* format, char* msg, size_t n) {
  if (!file || bytes <= 0) return bad(msg, n, "the file is empty");
  if (bytes < 20) return bad(msg, n, "the file ends inside its header (%lld bytes)", (long long)bytes);
  if (std::memcmp(file, "livox_file", 10) == 0) {
    *format = kFmtCsimLegacy;
  } else if (std::memcmp(file, "livox_tech", 10) == 0) {
    static const uint8_t v2[6] = {'2', '.', '0', '.', '0', 0}, v11[4] = {1, 1, 0, 0}, z6[6] = {0, 0, 0, 0, 0, 0};
    if (std::memcmp(file + 10, v2, 6) == 0) *format = kFmtCsimLvx2;
    else if (std::memcmp(file + 10, z6, 6) == 0 && std::memcmp(file + 16, v11, 4) == 0) *format = kFmtV11;
    else return bad(msg, n, "livox_tech file of an unknown version (neither 1.1.0.0 nor \"2.0.0\")");
  } else {
    return bad(msg, n, "unknown file signature (neither livox_tech nor livox_file)");
  }
  const int64_t hdr = file_header_bytes(*format);
  if (bytes < hdr)
    return bad(msg, n, "the file ends inside its %lld-byte header (%lld bytes)", (long long)hdr, (long long)bytes);
  if (*format != kFmtCsimLegacy) {
    const uint32_t magic = rd<uint32_t>(file + (*format == kFmtV11 ? 20 : 16));
    if (magic != kMagic) return bad(msg, n, "wrong magic code 0x%08X (0xAC0EA767 expected)", magic);
  }
  return 0;
}

// the walk: counts the frames; fills what is not null (at most cap frames)
int walk(const uint8_t* file, int64_t bytes, int format, int64_t cap, int32_t* n_frames, int64_t* frame_pos,
         int64_t* slots, uint64_t* ids, int64_t* ts, char* msg, size_t n) {
  int64_t F = 0;
  int64_t pos = file_header_bytes(format);
  const int64_t fh = frame_header_bytes(format);
  while (pos < bytes) {
    if (F >= INT32_MAX - 1) return bad(msg, n, "too many frames");
    if (bytes - pos < fh)
      return bad(msg, n, "frame %lld at byte %lld: the file ends inside the frame header", (long long)F, (long long)pos);
    int64_t next, nslots, t;
    uint64_t id;
    if (format == kFmtV11) {
      const uint64_t own = rd<uint64_t>(file + pos), nx = rd<uint64_t>(file + pos + 8);
      id = rd<uint64_t>(file + pos + 16);
      if (own != (uint64_t)pos)
        return bad(msg, n, "frame %lld at byte %lld stores its own offset as %llu", (long long)F, (long long)pos,
                   (unsigned long long)own);
      if (nx == 0) {
        next = bytes;   // the last frame runs to the end of the file
      } else {
        if (nx <= (uint64_t)pos)
          return bad(msg, n, "frame %lld: the next-frame offset %llu points backwards", (long long)F,
                     (unsigned long long)nx);
        if (nx >= (uint64_t)bytes)
          return bad(msg, n, "frame %lld: the next-frame offset %llu is past the end (%lld bytes)", (long long)F,
                     (unsigned long long)nx, (long long)bytes);
        next = (int64_t)nx;
      }
      const int64_t body = next - pos - fh;
      if (body < 0 || body % kV11Pkg != 0)
        return bad(msg, n, "frame %lld spans %lld bytes: not a header and whole 1366-byte packages%s", (long long)F,
                   (long long)(next - pos), nx == 0 ? " (file cut short?)" : "");
      nslots = body / kV11Pkg * kV11PkgPoints;
      t = body ? (int64_t)rd<uint64_t>(file + pos + fh + 14) : -1;
    } else {
      uint32_t count;
      if (format == kFmtCsimLegacy) {
        t = (int64_t)rd<uint64_t>(file + pos);
        count = rd<uint32_t>(file + pos + 8);
        id = (uint64_t)F;
      } else {
        id = rd<uint32_t>(file + pos);
        t = (int64_t)rd<uint64_t>(file + pos + 4);
        count = rd<uint32_t>(file + pos + 12);
      }
      if ((int64_t)count > (bytes - pos - fh) / kRec)
        return bad(msg, n, "frame %lld stores %u points but %lld bytes remain", (long long)F, count,
                   (long long)(bytes - pos - fh));
      nslots = count;
      next = pos + fh + kRec * (int64_t)count;
    }
    if (F < cap) {
      if (frame_pos) frame_pos[F] = pos;
      if (slots) slots[F] = nslots;
      if (ids) ids[F] = id;
      if (ts) ts[F] = t;
    }
    ++F;
    pos = next;
  }
  if (format == kFmtCsimLegacy) {
    const uint32_t stored = rd<uint32_t>(file + 14);
    if ((int64_t)stored != F)
      return bad(msg, n, "the header announces %u frames, the file holds %lld", stored, (long long)F);
  }
  if (frame_pos && F <= cap) frame_pos[F] = bytes;
  *n_frames = (int32_t)F;
  return 0;
}

}  // namespace

int64_t file_header_bytes(int format) {
  return format == kFmtV11 ? kV11FileHdr : format == kFmtCsimLegacy ? kLegacyFileHdr : format == kFmtCsimLvx2 ? kLvx2FileHdr : 0;
}
int64_t frame_header_bytes(int format) {
  return format == kFmtV11 ? kV11FrameHdr : format == kFmtCsimLegacy ? kLegacyFrameHdr : format == kFmtCsimLvx2 ? kLvx2FrameHdr : 0;
}

int probe(const uint8_t* file, int64_t bytes, int* format, int32_t* n_frames, char* msg, size_t n) {
  int fmt = -1;
  int32_t F = 0;
  if (int r = sniff(file, bytes, &fmt, msg, n)) return r;
  if (int r = walk(file, bytes, fmt, 0, &F, nullptr, nullptr, nullptr, nullptr, msg, n)) return r;
  if (format) *format = fmt;
  if (n_frames) *n_frames = F;
  return 0;
}

int index(const uint8_t* file, int64_t bytes, int format, int32_t n_frames, int64_t* frame_pos, int64_t* slots,
          uint64_t* frame_ids, int64_t* timestamp_ns, DeviceBlock* dev, char* msg, size_t n) {
  int fmt = -1;
  if (int r = sniff(file, bytes, &fmt, msg, n)) return r;
  if (fmt != format) return bad(msg, n, "the file is of format %d, not %d", fmt, format);
  if (n_frames < 0) return bad(msg, n, "negative frame count");
  int32_t F = 0;
  if (int r = walk(file, bytes, fmt, n_frames, &F, frame_pos, slots, frame_ids, timestamp_ns, msg, n)) return r;
  if (F != n_frames) return bad(msg, n, "the file holds %d frames, not %d", F, n_frames);
  if (dev) {
    std::memset(dev, 0, sizeof *dev);
    if (fmt == kFmtV11) {          // LMC:146-172: SN, hub SN, index, type, extrinsic enable, 6 floats
      std::memcpy(dev->sn, file + 29, 16);
      dev->device_type = file[62];
      dev->extrinsic_enable = file[63];
      std::memcpy(dev->extrinsics, file + 64, 24);
    } else if (fmt == kFmtCsimLegacy) {   // CSIM:302-306
      std::memcpy(dev->sn, file + 28, 16);
      dev->device_type = file[44];
    } else {                        // CSIM:332-339
      std::memcpy(dev->sn, file + 32, 16);
      dev->device_type = file[48];
      dev->extrinsic_enable = file[49];
      std::memcpy(dev->extrinsics, file + 50, 24);
    }
  }
  return 0;
}

int check_layout(int format, int64_t bytes, int32_t F, const int64_t* frame_pos, const int64_t* counts, char* msg,
                 size_t n) {
  const int64_t hdr = file_header_bytes(format), fh = frame_header_bytes(format);
  if (!hdr) return bad(msg, n, "unknown LVX format %d", format);
  if (F < 0 || !frame_pos) return bad(msg, n, "frame_pos is NULL or the frame count negative");
  if (bytes < hdr) return bad(msg, n, "the file is shorter than its header");
  if (frame_pos[0] != hdr || frame_pos[F] != bytes)
    return bad(msg, n, "frame_pos must run from the file header (%lld) to the file size (%lld)", (long long)hdr,
               (long long)bytes);
  if (format != kFmtV11 && F > 0 && !counts) return bad(msg, n, "counts is NULL");
  for (int32_t f = 0; f < F; ++f) {
    if (frame_pos[f] < hdr || frame_pos[f] > bytes || frame_pos[f + 1] > bytes || frame_pos[f + 1] - frame_pos[f] < fh)
      return bad(msg, n, "frame %d: positions not increasing inside the file", f);
    const int64_t body = frame_pos[f + 1] - frame_pos[f] - fh;
    if (format == kFmtV11) {
      if (body % kV11Pkg) return bad(msg, n, "frame %d: body of %lld bytes is not whole packages", f, (long long)body);
      const int64_t s = body / kV11Pkg * kV11PkgPoints;
      if (counts && (counts[f] < 0 || counts[f] > s))
        return bad(msg, n, "frame %d: count %lld outside its %lld record slots", f, (long long)counts[f], (long long)s);
    } else if (counts[f] < 0 || body != counts[f] * kRec) {
      return bad(msg, n, "frame %d: count %lld does not match its %lld body bytes", f, (long long)counts[f],
                 (long long)body);
    }
    if (counts && counts[f] >= ((int64_t)1 << 31)) return bad(msg, n, "frame %d has 2^31 points or more", f);
  }
  return 0;
}

}  // namespace mcingest
