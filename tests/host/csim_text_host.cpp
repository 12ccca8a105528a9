// Host build of the device text formatters behind the CSIM exports: the "%.6f" formatter
// (csrc/fmt6_core.hpp) and the "%.0f" formatter and line-descriptor prepare / emit
// (csrc/csim_text_core.hpp, which includes it), behind the host stand-ins for the few device builtins
// they use, for tests/test_csim_text_host.py.  Every value is compared with the C library's
// correctly rounded snprintf("%.0f") / ("%.6f") (the same digits as Python's formatting; a NaN prints
// "nan" whatever its sign, as Python does), then whole lines of the three descriptors (PCD, XYZ, CSV)
// are emitted back to back into a guarded buffer and compared.  Prints "bad <count>"; exit status
// = min(count, 255).
//   csim_text_host file <in> <out>   in: raw float64 values; out: per value one line, the texts of
//                                    fmt6_prepare, fmt0_prepare and csim_fmt6_prepare separated by tabs
//                                    ("range" for a value beyond the formatters).  The harness computes;
//                                    tests/test_corevalues_cpu.py compares.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "device_standins.hpp"
#include "csim_text_core.hpp"
using namespace mc;

static int bad = 0;

static std::string want_value(double v, bool dec0, bool nan_empty) {
  if (std::isnan(v)) return nan_empty ? "" : "nan";
  char b[96];
  std::snprintf(b, sizeof b, dec0 ? "%.0f" : "%.6f", v);
  return b;
}

static void check_value(double v) {
  for (int dec0 = 0; dec0 < 3; ++dec0) {   // "%.6f" of codecs.hpp, "%.0f", the lines' "%.6f" (csim_fmt6_*)
    const Fmt6 f = dec0 == 1 ? fmt0_prepare(v) : dec0 == 2 ? csim_fmt6_prepare(v) : fmt6_prepare(v);
    const bool out = std::isfinite(v) && std::fabs(v) >= std::ldexp(1.0, 107);
    if (out != (f.kind == 3)) { if (++bad < 20) std::printf("range flag of %a: kind %d\n", v, f.kind); continue; }
    if (out) continue;
    char got[96];
    std::memset(got, '#', sizeof got);
    if (dec0 == 1) fmt0_write(f, got + 1);
    else if (dec0 == 2) csim_fmt6_write(f, got + 1);
    else fmt6_write(f, got + 1);
    const std::string w = want_value(v, dec0 == 1, false);
    if (f.len != (int)w.size() || std::memcmp(got + 1, w.data(), w.size()) || got[0] != '#' || got[1 + f.len] != '#') {
      if (++bad < 20) std::printf("%s (%d) of %a: got [%.*s] len %d want [%s]\n", dec0 == 1 ? "%.0f" : "%.6f", dec0, v, f.len, got + 1, f.len, w.c_str());
    }
  }
}

// file mode: the three formatters' text of every value of a file, for the test to compare
static int file_mode(const char* in_path, const char* out_path) {
  FILE* in = std::fopen(in_path, "rb");
  FILE* out = std::fopen(out_path, "wb");
  if (!in || !out) return 2;
  double v;
  while (std::fread(&v, sizeof v, 1, in) == 1) {
    for (int which = 0; which < 3; ++which) {
      const Fmt6 f = which == 1 ? fmt0_prepare(v) : which == 2 ? csim_fmt6_prepare(v) : fmt6_prepare(v);
      char got[96];
      if (f.kind == 3) {
        std::fputs("range", out);
      } else {
        if (which == 1) fmt0_write(f, got);
        else if (which == 2) csim_fmt6_write(f, got);
        else fmt6_write(f, got);
        std::fwrite(got, 1, (size_t)f.len, out);
      }
      std::fputc(which < 2 ? '\t' : '\n', out);
    }
  }
  std::fclose(in);
  return std::fclose(out) ? 2 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "file")) return file_mode(argv[2], argv[3]);
  const int N = argc > 1 ? std::atoi(argv[1]) : 200000;
  std::mt19937_64 g(7);
  std::vector<double> vals = {0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -0.3, 0.3, -1.5, 3.5, 0.49999999999999994, 0.5000000000000001,
                              254.5, 255.5, 9007199254740994.0, 1.23e18, 1e22, 1e31, -1e31, 5e-324, -5e-324,
                              0.9999995, 9.9999995, 999.9999995, 0.0000005, 0.0000015, 0.0078125, 1e15 + 0.5, 4503599627370495.5,
                              4503599627370496.5, 9.5, 10.5, 99.5, 999999.5, 1.7e18, 1700000000000001000.0,
                              std::ldexp(1.0, 107), -std::ldexp(1.0, 107), std::nextafter(std::ldexp(1.0, 107), 0.0),
                              1e300, (double)INFINITY, -(double)INFINITY, std::nan(""), -std::nan(""),
                              // integers whose bits 32..95 are all zero (a 64-bit view of ip >> 32 took them for
                              // 32-bit values: "0.000000" and "6" for 2^100), and float32 values with as many zeros
                              std::ldexp(1.0, 96), std::ldexp(1.0, 100), -std::ldexp(1.0, 106), std::ldexp(2047.0, 96),
                              std::ldexp(1.0, 90), std::ldexp(3.0, 90), -0x1.62c7p+106, -0x1.8d4p+101, 0x1.fffffep+106};
  // random doubles over every exponent up to 2^107 (and a few beyond), random sign and mantissa
  for (int i = 0; i < N; ++i) {
    const uint64_t r = g();
    const uint64_t ex = (i % 97 == 0) ? 1023 + 107 + g() % 40 : g() % (1023 + 107);
    const uint64_t bits = (r & 0x800fffffffffffffull) | (ex << 52);
    double v;
    std::memcpy(&v, &bits, 8);
    vals.push_back(v);
  }
  // the LiDAR ranges: coordinates, intensities with halves, nanosecond timestamps, k + 1/2 ties
  std::uniform_real_distribution<double> U(-100, 100);
  for (int i = 0; i < N / 4; ++i) {
    vals.push_back(U(g));
    vals.push_back((double)(int64_t)(g() % 512) / 2.0);
    vals.push_back((double)(1700000000000000000ull + g() % 100000000000ull));
    vals.push_back(((double)(int64_t)(g() % (1ull << 52)) + 0.5) * (g() % 2 ? 1 : -1));
    // 4294 <= |v| < 2^64, the range csim_fmt6_prepare splits into integer and fraction: fractions at
    // and next to the sixth-decimal ties and the carry into the integer part, integers of every size
    const double I = (double)(g() % (1ull << (13 + g() % 40)));
    const double t = I + (double)(g() % 2000001) * 0.5e-6;
    vals.push_back(g() % 2 ? t : -t);
    vals.push_back(std::nextafter(t, g() % 2 ? 0.0 : 1e300));
    vals.push_back((double)(g() >> (g() % 52)));
    vals.push_back(I + 0.9999995 + 1e-9 * (double)((int)(g() % 2001) - 1000));
  }
  for (double v : {4293.9999995, 4294.0, 4294.0000005, 4294.9999995, 65536.0000005, 4503599627370495.5, 4503599627370496.0,
                   18446744073709549568.0, 18446744073709551616.0, 36893488147419103232.0, 1048576.0078125, 99999.9999995})
    for (double s : {1.0, -1.0}) vals.push_back(s * v);
  for (double v : vals) check_value(v);

  // whole lines: PCD "%.6f %.6f %.6f %.0f %.0f\n", XYZ "%.6f %.6f %.6f\n", CSV with empty NaN fields
  const CsimLine descs[3] = {{5, ' ', 0x18u, 0}, {3, ' ', 0u, 0}, {5, ',', 0u, 1}};
  long lines = 0;
  for (int d = 0; d < 3; ++d) {
    std::string want;
    std::vector<char> buf;
    std::vector<CsimText> L;
    std::vector<int> off;
    int err = 0, at = 0;
    const size_t rows = 20000;
    for (size_t i = 0; i < rows; ++i) {
      double c[5];
      for (int k = 0; k < 5; ++k) {
        c[k] = vals[(i * 5 + k + 11 * d) % vals.size()];
        if (std::isfinite(c[k]) && std::fabs(c[k]) >= std::ldexp(1.0, 107)) c[k] = 1.0;
      }
      CsimText t;
      csim_line_prepare(descs[d], c, t, &err);
      std::string w;
      for (int k = 0; k < descs[d].ncols; ++k)
        w += want_value(c[k], (descs[d].dec0 >> k) & 1, descs[d].nan_empty != 0) + (k + 1 < descs[d].ncols ? std::string(1, (char)descs[d].sep) : "\n");
      if (t.len != (int)w.size()) { if (++bad < 20) std::printf("line length %d want %zu: %s", t.len, w.size(), w.c_str()); }
      want += w;
      off.push_back(at);
      at += (int)w.size();
      L.push_back(t);
      ++lines;
    }
    buf.assign(want.size() + 32, '#');
    for (size_t i = rows; i-- > 0;) csim_line_emit(descs[d], L[i], buf.data() + 16 + off[i]);   // any order
    if (err) { ++bad; std::printf("descriptor %d: range error flag set\n", d); }
    if (std::memcmp(buf.data() + 16, want.data(), want.size())) {
      ++bad;
      size_t i = 0;
      while (buf[16 + i] == want[i]) ++i;
      std::printf("descriptor %d: byte %zu differs: want [%s]\n", d, i, want.substr(i > 30 ? i - 30 : 0, 80).c_str());
    }
    for (int i = 0; i < 16; ++i)
      if (buf[i] != '#' || buf[16 + want.size() + i] != '#') { ++bad; std::printf("descriptor %d: guard byte written\n", d); break; }
  }
  // a value beyond the range sets the error flag
  {
    int err = 0;
    double c[5] = {1, 2, 3, 4, std::ldexp(1.0, 107)};
    CsimText t;
    csim_line_prepare(descs[0], c, t, &err);
    if (!err) { ++bad; std::printf("2^107 did not set the error flag\n"); }
  }
  std::printf("values %zu lines %ld bad %d\n", vals.size(), lines, bad);
  return bad > 255 ? 255 : bad;
}
