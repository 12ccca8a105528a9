// Host build of the device text-token parser behind the ingest decoders (csrc/ingest_token_core.hpp), for
// tests/test_ingest_host.py.  Every in-window token is compared bit for bit with the C library's correctly rounded
// strtod (Python's float()); out-of-window tokens must be flagged and carry no value.  argv[1] =
// random tokens per (significant digits, fractional digits) pair.  Prints "bad <count>"; exit status
// = min(count, 255).
//   ingest_host file <in> <out>   in: newline-separated tokens; out: per token the value's bits (u64), bad
//                                 and len (i32 each), parsed with a ' ' separator behind the token.  The
//                                 harness computes; tests/test_corevalues_cpu.py compares.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ingest_token_core.hpp"
using namespace mc;

static int bad = 0;
static long checked = 0;

static uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

// the token in a guarded copy: followed by the separator / newline / nothing, never by a NUL the parser could lean on
static IngestTok parse(const std::string& tok, char sep, bool empty_nan, int tail) {
  std::string buf = "#" + tok + (tail == 0 ? std::string(1, sep) + "7" : tail == 1 ? "\n9" : tail == 2 ? "\r\n" : "");
  const char* p = buf.data() + 1;
  const char* e = buf.data() + buf.size();
  return ingest_token(p, e, sep, empty_nan);
}

static void want_value(const std::string& tok) {
  const double w = std::strtod(tok.c_str(), nullptr);
  for (int tail = 0; tail < 4; ++tail) {
    const IngestTok t = parse(tok, tail & 1 ? ',' : ' ', false, tail);
    ++checked;
    const bool same = std::isnan(w) ? std::isnan(t.v) : bits_of(t.v) == bits_of(w);
    if (t.bad || t.len != (int)tok.size() || !same) {
      if (++bad < 30) std::printf("token [%s]: bad %d len %d got %a want %a\n", tok.c_str(), t.bad, t.len, t.v, w);
      return;
    }
  }
}

static void want_flag(const std::string& tok) {
  for (int tail = 0; tail < 4; ++tail) {
    const IngestTok t = parse(tok, ' ', false, tail);
    ++checked;
    if (!t.bad || t.v != 0.0) {
      if (++bad < 30) std::printf("token [%s] outside the window: bad %d value %a\n", tok.c_str(), t.bad, t.v);
      return;
    }
  }
}

// the window, restated on the text: [+-]digits[.digits] with at most 19 significant and 19 fractional digits
// after stripping the sign, the leading zeros and the fraction's trailing zeros
static bool in_window(std::string t) {
  if (!t.empty() && (t[0] == '-' || t[0] == '+')) t.erase(0, 1);
  const size_t dot = t.find('.');
  std::string ip = t.substr(0, dot), fr = dot == std::string::npos ? "" : t.substr(dot + 1);
  while (!fr.empty() && fr.back() == '0') fr.pop_back();
  std::string all = ip + fr;
  all.erase(0, all.find_first_not_of('0') == std::string::npos ? all.size() : all.find_first_not_of('0'));
  return fr.size() <= 19 && all.size() <= 19;
}
static void check(const std::string& tok) { if (in_window(tok)) want_value(tok); else want_flag(tok); }

// M (nsig digits, the first not zero) with the point k digits from the right
static std::string make(const std::string& digits, int k) {
  const int n = (int)digits.size();
  if (k == 0) return digits;
  if (k >= n) return "0." + std::string(k - n, '0') + digits;
  return digits.substr(0, n - k) + "." + digits.substr(n - k);
}

// file mode: every token of a file parsed in place (the '\n' behind it ends it), for the test to compare
static int file_mode(const char* in_path, const char* out_path) {
  std::string text;
  if (FILE* in = std::fopen(in_path, "rb")) {
    char buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, in)) > 0) text.append(buf, k);
    std::fclose(in);
  } else {
    return 2;
  }
  FILE* out = std::fopen(out_path, "wb");
  if (!out) return 2;
  const char* e = text.data() + text.size();
  for (const char* p = text.data(); p < e;) {
    const char* nl = (const char*)std::memchr(p, '\n', (size_t)(e - p));
    const IngestTok t = ingest_token(p, e, ' ', false);
    struct { uint64_t bits; int32_t bad, len; } o = {bits_of(t.v), t.bad, t.len};
    static_assert(sizeof o == 16, "packed");
    std::fwrite(&o, sizeof o, 1, out);
    p = nl ? nl + 1 : e;
  }
  return std::fclose(out) ? 2 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "file")) return file_mode(argv[2], argv[3]);
  const int per = argc > 1 ? std::atoi(argv[1]) : 530;
  std::mt19937_64 rng(20240607);
  // every significant-digit count 1..19 with every fractional length 0..19
  for (int nsig = 1; nsig <= 19; ++nsig)
    for (int k = 0; k <= 19; ++k)
      for (int r = 0; r < per; ++r) {
        std::string d(nsig, '0');
        for (int i = 0; i < nsig; ++i) d[i] = (char)('0' + rng() % 10);
        if (d[0] == '0') d[0] = (char)('1' + rng() % 9);
        if (k > 0 && d[nsig - 1] == '0') d[nsig - 1] = (char)('1' + rng() % 9);   // k is the stripped fraction length
        if (r % 7 == 0) for (int i = nsig / 2; i < nsig - 1; ++i) d[i] = r % 14 ? '9' : '0';   // long carries, sticky-only tails
        std::string t = make(d, k);
        const int dress = (int)(rng() % 8);
        if (dress & 1) t = std::string(1 + rng() % 3, '0') + t;                              // leading zeros
        if (dress & 2) t += (k == 0 ? "." : "") + std::string(rng() % 7, '0');              // trailing zeros / "5."
        if (dress & 4) t = (rng() & 1 ? "-" : "+") + t;
        want_value(t);
      }
  // planted
  const char* ints[] = {"9007199254740991", "9007199254740992", "9007199254740993", "9007199254740995",
                        "9223372036854776832", "18446744073709551615", "9007199254740994", "9007199254740997",
                        "1700000000000000000", "9999999999999999999", "0", "1", "4503599627370497"};
  for (const char* s : ints) {
    check(s);
    check(std::string(s) + ".000000");
    check(std::string(s) + ".");
    check(std::string("-") + s);
    const std::string t(s);
    if (t.size() > 3) {   // the same digits with a fraction
      for (size_t cut = 1; cut < t.size(); ++cut) check(t.substr(0, cut) + "." + t.substr(cut));
      check("0." + t);
      check("0.0" + t.substr(0, 18));
    }
  }
  const char* vals[] = {"0.500000", "1.500000", "2.500000", "0.000005", "0.000015", "0.000025", "123456.500000", "0.125000",
                        "4294.967295", "4294.967296", "0.000001", "0.000000", "-0.000000", "-0", "+0.0", "000.000100",
                        "0001", "00012.3400", "5.", "-5.", "100", "1000000", "10.010", "0.1", "0.3", "2.675", "1.005",
                        "0.0000000000000000001", "0.9999999999999999999", "9.999999999999999999", "1844674407370955.1615",
                        "9007199254740993.0", "9007199254740992.5", "9007199254740993.5", "900719925474099.35",
                        "90071992547409.925", "4503599627370496.5", "4503599627370497.5", "9223372036854775807.000000",
                        "nan", "inf", "-inf", "+inf"};
  for (const char* s : vals) check(s);
  {   // sign of zero
    const IngestTok t = parse("-0.000000", ' ', false, 1);
    if (t.bad || !std::signbit(t.v) || t.v != 0.0) { ++bad; std::printf("-0.000000 -> %a\n", t.v); }
  }
  {   // the empty CSV field
    const IngestTok t = parse("", ',', true, 0), u = parse("", ',', false, 0);
    if (t.bad || !std::isnan(t.v) || t.len != 0) { ++bad; std::printf("empty CSV field: bad %d value %a\n", t.bad, t.v); }
    if (!u.bad) { ++bad; std::printf("empty field without empty_nan not flagged\n"); }
  }
  const char* outside[] = {"12345678901234567890", "1e5", "1.2.3", "--1", "abc", "1.23e-4", ".5", "-", "+", "-nan", "nanx",
                           "infinity", "1,5x", "0x10", "1.00000000000000000001", "0.00000000000000000001", "12a", "1 ",
                           "18446744073709551616", "99999999999999999999", "1234567890123456789.5", "in", "na", "1_0"};
  for (const char* s : outside) {
    if (std::string(s).find(' ') != std::string::npos || std::string(s).find(',') != std::string::npos) continue;
    want_flag(s);
  }
  // whole lines
  struct L { const char* text; char sep; int n; bool en; int want; } lines[] = {
      {"1.5 2.5 -3.25\n", ' ', 3, false, 0},          {"1.5 2.5 -3.25", ' ', 3, false, 0},
      {"1.5 2.5 -3.25\r\n", ' ', 3, false, 0},        {"1.5 2.5\n", ' ', 3, false, kIngestBadFields},
      {"1.5 2.5 3 4\n", ' ', 3, false, kIngestBadFields}, {"1,,3,4,5\n", ',', 5, true, 0},
      {",,,,\n", ',', 5, true, 0},                    {"1,2,3,4\n", ',', 5, true, kIngestBadFields},
      {"1 2 1e5\n", ' ', 3, false, kIngestBadToken},  {"1  2 3\n", ' ', 3, false, kIngestBadToken},
      {"1 2 3\rx\n", ' ', 3, false, kIngestBadFields}, {"1 2 3 4 5 6 7 8\n", ' ', 8, false, 0}};
  for (const L& l : lines) {
    double v[kIngestMaxCols];
    const std::string s = std::string("#") + l.text;
    const int got = ingest_line(s.data() + 1, s.data() + s.size(), l.sep, l.n, l.en, v);
    ++checked;
    if (got != l.want) { ++bad; std::printf("line [%s]: %d, want %d\n", l.text, got, l.want); }
  }
  {
    double v[kIngestMaxCols];
    const std::string s = "1,,3.5,,1700000000000000000.000000\n";
    if (ingest_line(s.data(), s.data() + s.size(), ',', 5, true, v) != 0 || v[0] != 1.0 || !std::isnan(v[1]) || v[2] != 3.5 ||
        !std::isnan(v[3]) || v[4] != 1.7e18) { ++bad; std::printf("CSV line values\n"); }
  }
  std::printf("checked %ld\nbad %d\n", checked, bad);
  return bad > 255 ? 255 : bad;
}
