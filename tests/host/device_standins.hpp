// device_standins.hpp — the host's one stand-in for each device builtin that the text of a core header
// (csrc/*_core.hpp, unit_order.hpp) uses.  A harness includes this first, then the core.  The library's own
// headers never include it.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <math.h>

// the device's address-space attribute (the LDS pointer of pcd_line_core.hpp) means nothing here
#pragma GCC diagnostic ignored "-Wattributes"

using std::fabs;
using std::floor;
using std::fma;
using std::ldexp;
using std::rint;
using std::signbit;

static inline long long __double_as_longlong(double v) { long long b; std::memcpy(&b, &v, 8); return b; }
static inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
// v_mul_i32_i24: the low 24 bits of each operand as signed integers
static inline int __mul24(int a, int b) {
  const int64_t x = (int64_t)(int32_t)((uint32_t)a << 8) >> 8, y = (int64_t)(int32_t)((uint32_t)b << 8) >> 8;
  return (int)(uint32_t)(uint64_t)(x * y);
}
// v_perm_b32: byte i of the result = byte sel[i] of {s0:s1} (0-3 = s1, 4-7 = s0), 12 -> 0x00
static inline uint32_t __builtin_amdgcn_perm(uint32_t s0, uint32_t s1, uint32_t sel) {
  const uint64_t v = ((uint64_t)s0 << 32) | s1;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t c = (sel >> (8 * i)) & 0xffu;
    const uint32_t b = c < 8 ? (uint32_t)(v >> (8 * c)) & 0xffu : (c == 12 ? 0u : 0xffu);
    r |= b << (8 * i);
  }
  return r;
}
// ds_or_b64 / ds_or_b32 (an LDS atomic OR): the host's plain read-modify-write
#ifndef __ATOMIC_RELAXED
#define __ATOMIC_RELAXED 0
#endif
#define __HIP_MEMORY_SCOPE_WORKGROUP 0
template <class T>
static inline T __hip_atomic_fetch_or(T* p, T v, int, int) {
  T o;
  std::memcpy(&o, p, sizeof o);
  const T n = o | v;
  std::memcpy(p, &n, sizeof n);
  return o;
}
struct alignas(16) uint4 { uint32_t x, y, z, w; };   // HIP's 16-byte vector: the kernels' text chunks
