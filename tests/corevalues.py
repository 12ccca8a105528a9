"""Seeded value classes for the scalar cores under the text writers, the text parser and the LAS codec,
with each core's branch conditions restated on the value or on the text (numpy / Python only, nothing
of the package is called).  tests/test_corevalues_cpu.py feeds them to the g++ builds of the cores and
counts the branches; tests/test_gpu_corevalues.py sends the same values through the kernels, where
hipcc's own lowering of the same source runs (fused multiply-adds, inline 128-bit division, its
uint64 -> double conversion, ldexp, rint, floor, denormals).

Formatter classes (float64): F1 |v| < 4294, F2 4294 <= |v| < 2^52, F3 integers 2^52 <= |v| < 2^64,
F4 2^64 <= |v| < 2^107, F5 |v| < 1e-6, F6 the "%.0f" ties and binades, F7 NaN / inf / zeros.
Token classes (bytes): P1 every (significant digits, fraction length) pair, P2 decimal midpoints
between adjacent doubles, P3 the planted lists of tests/host/ingest_host.cpp, P4 "%.6f" round trips.
LAS classes: rows and (scale, offset) pairs with quotient ties, the int32 edges, the intensity edges
and gps times off the nanosecond grid.  Every generator takes a seed and a size.
"""
import math
from fractions import Fraction

import numpy as np

INF = float("inf")
TILE_LINES = 256            # lines per workgroup of k_csim_text_write and of k_text_parse
TILE_TEXT = 256 * 96        # kCsimTileText = kTextLds: LDS text bytes per tile


def _signed(rng, a):
    return a * rng.choice([-1.0, 1.0], len(a))


def _around(a):
    """each value, then its two float64 neighbours"""
    a = np.asarray(a, np.float64)
    return np.concatenate([a, np.nextafter(a, -INF), np.nextafter(a, INF)])


# ---- formatter classes ---------------------------------------------------------------------------------
def f1(seed, n):
    """|v| < 4294: uniform values, exact sixth-decimal ties (k / 128, k / 64), near-ties
    float((m + 0.5) * 1e-6) with both neighbours."""
    rng = np.random.default_rng(seed)
    q = max(n // 9, 1)
    uni = rng.uniform(0.0, 4293.99, 3 * q)
    k = rng.integers(0, 4293 * 64, 2 * q) * 2 + 1
    dy = np.concatenate([k[:q] / 128.0, k[q:] / 64.0 / (2.0 ** rng.integers(0, 6, q))])
    m = rng.integers(0, 4293_000_000, q)
    near = _around((m + 0.5) * 1e-6)
    v = np.concatenate([uni, dy, near, [4293.9999995, 0.9999995, 9.9999995, 999.9999995, 0.0000005, 0.0000015, 0.0078125]])
    v = v[v < 4294.0]
    return _signed(rng, v)


def f2(seed, n):
    """4294 <= |v| < 2^52, the binades 12..51 evenly: I + j * 0.5e-6 (j in 0..2 000 000) with both
    neighbours, I + 0.9999995 +- d (the carry into the integer part), I + 2^-b dyadics."""
    rng = np.random.default_rng(seed)
    q = max(n // 6, 40)
    b = 12 + np.arange(q) % 40
    lo = np.where(b == 12, 4294, 2.0 ** b).astype(np.int64)
    I = (lo + (rng.random(q) * (2.0 ** (b + 1) - 1 - lo)).astype(np.int64)).astype(np.float64)
    t = _around(I + rng.integers(0, 2_000_001, q) * 0.5e-6)
    carry = I + 0.9999995 + 1e-9 * rng.integers(-1000, 1001, q)
    dy = I + 2.0 ** -rng.integers(1, 40, q).astype(np.float64)
    fix = [4294.0, 4294.0000005, 4294.9999995, 65536.0000005, 1048576.0078125, 99999.9999995, 4503599627370495.5,
           1e15 + 0.5, 2.0 ** 32 - 1, 2.0 ** 32 + 1]
    v = np.concatenate([t, carry, dy, fix])
    v = v[(v >= 4294.0) & (v < 2.0 ** 52)]
    return _signed(rng, v)


def f3(seed, n):
    """integers 2^52 <= |v| < 2^64: random mantissas in every binade, float(10^k) with both neighbours
    (k = 16..19), 2^53 +- 2, the largest double below 2^64."""
    rng = np.random.default_rng(seed)
    b = 52 + np.arange(n) % 12
    v = np.ldexp((2 ** 52 + rng.integers(0, 2 ** 52, n)).astype(np.float64), b - 52)
    fix = np.concatenate([_around([float(10 ** k) for k in range(16, 20)]),
                          [2.0 ** 53 - 2, 2.0 ** 53 + 2, 2.0 ** 52, np.nextafter(2.0 ** 64, 0), 1.7e18, 1700000000000001000.0]])
    return _signed(rng, np.concatenate([v, fix]))


def f4(seed, n):
    """2^64 <= |v| < 2^107 (the 128-bit paths): random mantissas in every binade, a quarter of them with
    the 24 bits of a float32 (long runs of zero bits in N and in the integer part: a multiple of 2^96
    has bits 32..95 all zero), every power of two, the largest double and the largest float32 below
    2^107."""
    rng = np.random.default_rng(seed)
    b = 64 + np.arange(n) % 43
    m = 2 ** 52 + rng.integers(0, 2 ** 52, n)
    short = np.arange(n) // 43 % 4 == 0
    m[short] &= ~np.int64(2 ** 29 - 1)
    v = np.ldexp(m.astype(np.float64), b - 52)
    fix = [1e22, 1e31, 36893488147419103232.0, np.nextafter(2.0 ** 107, 0), float.fromhex("0x1.fffffep+106"),
           float.fromhex("0x1.62c7p+106"), float.fromhex("0x1.8d4p+101"), 2047 * 2.0 ** 96]
    return _signed(rng, np.concatenate([v, 2.0 ** np.arange(64, 107), fix]))


def f5(seed, n):
    """|v| < 1e-6: every binade from 2^-20 down through the denormals, 5e-324 and the largest denormal."""
    rng = np.random.default_rng(seed)
    e = -20 - np.arange(n) % 1055                      # -20 .. -1074
    frac = 1.0 + rng.random(n)
    v = np.ldexp(frac, e.astype(np.int64))             # below 2^-1022 this rounds into the denormals
    v = v[v < 1e-6]
    return _signed(rng, np.concatenate([v, [5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 9.999999e-7]]))


def f6(seed, n):
    """the "%.0f" class: k + 0.5 for even and odd k < 2^52 (both signs), every binade from -54 to 106,
    0.49999999999999994 and 0.5000000000000001."""
    rng = np.random.default_rng(seed)
    q = max(n // 2, 161)
    k = (rng.random(q) * 2.0 ** rng.integers(1, 53, q)).astype(np.int64)
    k[0::2] &= ~np.int64(1)
    k[1::2] |= np.int64(1)
    ties = k.astype(np.float64) + 0.5                  # exact below 2^52
    b = -54 + np.arange(q) % 161
    bin_ = np.ldexp(1.0 + rng.random(q), b.astype(np.int64))
    fix = [0.49999999999999994, 0.5000000000000001, 0.5, 1.5, 2.5, 3.5, 254.5, 255.5, 4503599627370495.5, 0.3]
    return _signed(rng, np.concatenate([ties, bin_, fix]))


def f7(seed=0, n=0):
    """NaN, -NaN, +-inf, +-0.0"""
    return np.array([np.nan, -np.nan, INF, -INF, 0.0, -0.0])


FORMATTER_CLASSES = (f1, f2, f3, f4, f5, f6, f7)


def formatter_pools(seed, n):
    """The seven classes, about n values each (F7 is its six values)."""
    return [g(seed + 11 * i, n) for i, g in enumerate(FORMATTER_CLASSES)]


def formatter_rows(seed, n_rows):
    """(n_rows, 5) float64 rows from F1..F7 in tiles of 256 lines.  Tile t mod 4: 0 = F1 and F5 only
    (short lines: staged, all below 4294); 1 = one class per column, rotated by the tile (every class
    in every column, F6 in columns 3 and 4 among them); 2 = the classes rotated per row (F4 mixed into
    tiles of short lines); 3 = F6 in columns 3 and 4, the PCD "%.0f" columns, F1 / F2 / F3 before them."""
    pools = formatter_pools(seed, max(n_rows // 4, 2000))
    at = [0] * 7

    def take(c, k):
        p = pools[c]
        idx = (at[c] + np.arange(k)) % len(p)
        at[c] += k
        return p[idx]

    rows = np.empty((n_rows, 5))
    for t, r0 in enumerate(range(0, n_rows, TILE_LINES)):
        k = min(TILE_LINES, n_rows - r0)
        kind, rot = t % 4, t // 4
        for c in range(5):
            if kind == 0:
                col = take(0 if (c + rot) % 3 else 4, k)
            elif kind == 1:
                col = take((c + rot) % 7, k)
            elif kind == 2:
                cls = (c + rot + np.arange(k)) % 7
                col = np.empty(k)
                for j in range(7):
                    col[cls == j] = take(j, int((cls == j).sum()))
            else:
                col = take(5 if c >= 3 else (c + rot) % 3, k)
            rows[r0:r0 + k, c] = col
    return rows


# ---- formatter branch predicates -------------------------------------------------------------------------
def _n64_edge():
    """the smallest double whose N = round-half-even(v * 10^6) does not fit 64 bits"""
    x = 18446744073709.551616
    while round(Fraction(x) * 1000000) >= 2 ** 64:
        x = float(np.nextafter(x, 0))
    return float(np.nextafter(x, INF))


N64_EDGE = _n64_edge()


def fmt6_branch(v):
    """The path fmt6_prepare (codecs.hpp) takes: 'fast' | 'exact' (|v| < 4294 within 1e-6 of a
    sixth-decimal tie) | 'wide' (4294 <= |v|, N = round(|v| 10^6) below 2^64) | 'wide128' (N >= 2^64) |
    'special'."""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    out = np.full(v.shape, "special", dtype=object)
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore", over="ignore"):
        y = a * 1000000.0
        fr = y - np.floor(y)
        near = np.abs(fr - 0.5) <= 1e-6
    small = fin & (a < 4294.0)
    out[small & ~near] = "fast"
    out[small & near] = "exact"
    big = fin & (a >= 4294.0)
    out[big & (a < N64_EDGE)] = "wide"
    out[big & (a >= N64_EDGE)] = "wide128"
    return out


def csim_fmt6_branch(v):
    """The path csim_fmt6_prepare (csim_codecs.hpp) takes: fmt6_prepare's below 4294 and from 2^64,
    'split' for 4294 <= |v| < 2^52, 'int' for 2^52 <= |v| < 2^64."""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    out = fmt6_branch(v)
    out[np.isfinite(v) & (a >= 4294.0) & (a < 2.0 ** 52)] = "split"
    out[np.isfinite(v) & (a >= 2.0 ** 52) & (a < 2.0 ** 64)] = "int"
    return out


def digit_groups(v, dec0):
    """put_digits' 9-digit groups for the integer part of one printed value: 0 where put_digits is not
    reached ("%.6f" with an integer part below 2^32, specials) or takes its 128-bit loop (4)."""
    v = float(v)
    if not math.isfinite(v):
        return 0
    text = ("%.0f" if dec0 else "%.6f") % abs(v)
    ip = int(text.split(".")[0])
    if ip >= 2 ** 64:
        return 4
    if not dec0 and ip < 2 ** 32:
        return 0
    return (len(str(ip)) + 8) // 9


def writer_tile_direct(lines, shift0=0):
    """Per tile of 256 lines: does k_csim_text_write take its direct path (text + shift > 256 * 96)?
    -> (direct flags, shifts), for one frame whose text starts at byte shift0."""
    direct, shifts, at = [], [], shift0
    for t in range(0, len(lines), TILE_LINES):
        total = sum(len(ln) for ln in lines[t:t + TILE_LINES])
        shifts.append(at & 15)
        direct.append(total + (at & 15) > TILE_TEXT)
        at += total
    return direct, shifts


# ---- token classes -----------------------------------------------------------------------------------------
def _make(digits, k):
    n = len(digits)
    if k == 0:
        return digits
    if k >= n:
        return "0." + "0" * (k - n) + digits
    return digits[:n - k] + "." + digits[n - k:]


def p1(seed, per, ints=0):
    """`per` random digit strings for every significant-digit count 1..19 and stripped fraction length
    0..19, dressed as tests/host/ingest_host.cpp dresses them: long runs of 9 / of 0, leading zeros,
    trailing fractional zeros, a bare trailing '.', '+' / '-'; `ints` more for the integers of 17..19
    digits (k == 0 with M >= 2^53: the conversion path, which only these three pairs reach)."""
    rng = np.random.default_rng(seed)
    out = []
    for nsig in range(1, 20):
        for k in range(20):
            for r in range(per + (ints if k == 0 and nsig >= 17 else 0)):
                d = [str(x) for x in rng.integers(0, 10, nsig)]
                if d[0] == "0":
                    d[0] = str(rng.integers(1, 10))
                if k > 0 and d[-1] == "0":
                    d[-1] = str(rng.integers(1, 10))
                if r % 7 == 0:
                    for i in range(nsig // 2, nsig - 1):
                        d[i] = "9" if r % 14 else "0"
                t = _make("".join(d), k)
                dress = int(rng.integers(0, 8))
                if dress & 1:
                    t = "0" * int(rng.integers(1, 4)) + t
                if dress & 2:
                    t += ("." if k == 0 else "") + "0" * int(rng.integers(0, 7))
                if dress & 4:
                    t = ("-" if rng.integers(0, 2) else "+") + t
                out.append(t.encode())
    return out


P2_CLASSES = ((52, 53, 1), (51, 52, 2), (50, 51, 3), (49, None, 4))   # binade of n, fraction bits of the midpoint


def p2(seed, per):
    """Decimal midpoints between adjacent doubles, `per` of each class and parity, each with its last
    digit +-1 (no tie: the sticky bit decides): n.5 for n in [2^52, 2^53), n.25 / n.75 for [2^51, 2^52),
    odd eighths for [2^50, 2^51), odd sixteenths for [2^49, 10^15) (19 digits)."""
    rng = np.random.default_rng(seed)
    ties, off = [], []
    for lo, hi, bits in P2_CLASSES:
        top = 2 ** hi if hi else 10 ** 15
        for i in range(per):
            n = int(rng.integers(2 ** lo, top - 1)) & ~1 | (i & 1)
            odd = 2 * int(rng.integers(0, 2 ** (bits - 1))) + 1
            frac = str(odd * 10 ** bits // 2 ** bits).rjust(bits, "0")    # odd / 2^bits, exactly `bits` decimals, ends in 5
            sign = "-" if i % 3 == 0 else ""
            ties.append(f"{sign}{n}.{frac}".encode())
            off.append(f"{sign}{n}.{frac[:-1]}4".encode())
            off.append(f"{sign}{n}.{frac[:-1]}6".encode())
    return ties, off


def is_exact_tie(tok):
    """fractions.Fraction: the token lies exactly half way between two adjacent doubles."""
    x = Fraction(tok.decode())
    f = float(tok)
    d = x - Fraction(f)
    if d == 0:
        return False
    other = float(np.nextafter(f, INF if d > 0 else -INF))
    return 2 * x == Fraction(f) + Fraction(other)


# the planted lists of tests/host/ingest_host.cpp, verbatim, less the two entries with 20 significant
# digits ("18446744073709551615", "1844674407370955.1615"): outside the window, the existing tests' subject
P3_INTS = ["9007199254740991", "9007199254740992", "9007199254740993", "9007199254740995", "9223372036854776832",
           "9007199254740994", "9007199254740997", "1700000000000000000", "9999999999999999999", "0", "1",
           "4503599627370497"]
P3_VALS = ["0.500000", "1.500000", "2.500000", "0.000005", "0.000015", "0.000025", "123456.500000", "0.125000",
           "4294.967295", "4294.967296", "0.000001", "0.000000", "-0.000000", "-0", "+0.0", "000.000100",
           "0001", "00012.3400", "5.", "-5.", "100", "1000000", "10.010", "0.1", "0.3", "2.675", "1.005",
           "0.0000000000000000001", "0.9999999999999999999", "9.999999999999999999",
           "9007199254740993.0", "9007199254740992.5", "9007199254740993.5", "900719925474099.35",
           "90071992547409.925", "4503599627370496.5", "4503599627370497.5", "9223372036854775807.000000",
           "nan", "inf", "-inf", "+inf"]


def p3(seed=0, n=0):
    out = []
    for s in P3_INTS:
        out += [s, s + ".000000", s + ".", "-" + s]
    return [t.encode() for t in out + P3_VALS]


def p4(seed, n):
    """"%.6f" % v for |v| < 10^13 from F1 / F2: the writers' own output, inside the window by
    construction (at most 13 + 6 digits)."""
    v = np.concatenate([f1(seed, n // 2), f2(seed + 1, n // 2)])
    v = v[np.abs(v) < 1e13]
    return [b"%.6f" % x for x in v.tolist()], v


def token_pools(seed, per=30, ints=700, ties=400, trips=4000):
    t2, o2 = p2(seed + 2, ties)
    return {"P1": p1(seed + 1, per, ints), "P2": t2, "P2off": o2, "P3": p3(), "P4": p4(seed + 4, trips)[0]}


# ---- token branch predicates (on the text) -----------------------------------------------------------------
def token_mk(tok):
    """-> (M, k) of a numeric token: sign, leading zeros and the fraction's trailing zeros stripped,
    the value is M / 10^k; None for nan / inf."""
    t = tok.lstrip(b"+-")
    if t in (b"nan", b"inf"):
        return None
    ip, _, fr = t.partition(b".")
    fr = fr.rstrip(b"0")
    return int(ip + fr), len(fr)


def token_branch(tok):
    """'special' | 'small' (M < 2^53: one IEEE division) | 'int' (k == 0: one conversion) | 'div'
    (ingest_div), then ingest_div's s and sh."""
    mk = token_mk(tok)
    if mk is None:
        return "special", None, None
    M, k = mk
    if M < 2 ** 53:
        return "small", None, None
    if k == 0:
        return "int", None, None
    D = 10 ** k
    s = 55 - M.bit_length() + D.bit_length()
    Q = (M << s) // D if s >= 0 else M // (D << -s)
    return "div", s, Q.bit_length() - 53


def text_body(tokens, ncols, sep=b" ", eol=b"\n", final=True):
    """The tokens laid out ncols to a line (the last line filled up with b"1"); with sep b"," every
    17th field is left empty (NaN).  -> (body, lines)"""
    toks = list(tokens)
    if sep == b",":
        for i in range(5, len(toks), 17):
            toks.insert(i, b"")
    toks += [b"1"] * (-len(toks) % ncols)
    lines = [sep.join(toks[i:i + ncols]) for i in range(0, len(toks), ncols)]
    body = eol.join(lines) + (eol if final else b"")
    return body, lines


def parser_tile_staged(lines, eol=1):
    """Per tile of 256 lines of a body without blank lines: does k_text_parse stage the tile in LDS
    (G1 - G0 + (G0 & 15) <= 256 * 96)?  -> (staged flags, shifts); eol = bytes ending a line."""
    staged, shifts, at = [], [], 0
    for t in range(0, len(lines), TILE_LINES):
        span = sum(len(ln) + eol for ln in lines[t:t + TILE_LINES])
        shifts.append(at & 15)
        staged.append(span + (at & 15) <= TILE_TEXT)
        at += span
    return staged, shifts


# ---- LAS classes -----------------------------------------------------------------------------------------
LAS_SCALES = (0.01, 0.001, 1e-6, 0.5, 3.0, 1.0 / 3.0, 0.007)
LAS_OFFSETS = (0.0, 500000.0, -3.25)
LAS_EDGE_Q = (-2.0 ** 31 - 1, -2.0 ** 31, 2.0 ** 31 - 1, 2.0 ** 31)


def las_quotient(v, scale, off):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(v, np.float64) - off) / scale


def _walk(v, steps):
    out = [v]
    lo = hi = v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        out += [lo, hi]
    return np.concatenate(out)


def las_coords(seed, n, scale, off):
    """-> (random values inside int32, quotient ties off + (k + 0.5) * scale with both neighbours, the
    int32 edges: values whose numpy quotient rounds to -2^31 - 1, -2^31, 2^31 - 1 or 2^31, the two .5
    ties among them)."""
    rng = np.random.default_rng(seed)
    rnd = off + rng.uniform(-2.0 ** 31 + 2, 2.0 ** 31 - 2, n) * scale
    k = rng.integers(-2 ** 30, 2 ** 30, n).astype(np.float64) // 2.0 ** rng.integers(0, 28, n)
    ties = _around(off + (k + 0.5) * scale)
    c = np.concatenate([np.arange(-2.0 ** 31 - 1.5, -2.0 ** 31 + 1, 0.5), np.arange(2.0 ** 31 - 1.5, 2.0 ** 31 + 1, 0.5)])
    cand = _walk(off + c * scale, 6)
    # the value whose quotient is the tie exactly, where float64 holds one (v = q * scale + off need not be it)
    edge = cand[np.isin(np.rint(las_quotient(cand, scale, off)), LAS_EDGE_Q)]
    return rnd, ties, np.unique(edge)


def las_intensities(imul):
    """column-3 values whose product with imul is -1, nextafter(-1, 0), the largest double below 65536,
    65536 (refused, accepted, accepted, refused), found among the neighbours of target / imul"""
    out = []
    for target in (-1.0, float(np.nextafter(-1.0, 0)), float(np.nextafter(65536.0, 0)), 65536.0):
        c = _walk(np.array([target / imul]), 3)
        hit = c[c * imul == target]
        if not len(hit):   # the product steps over the target (imul 65535): the nearest product on the accepted side
            inside = c[(c * imul > -1.0) & (c * imul < 65536.0)]
            hit = inside[np.argsort(np.abs(inside * imul - target))]
        out.append(hit[0])
    return np.array(out)


def las_rows(seed, n, scale, off, variant):
    """(rows (N, 5), the class of each row): every coordinate value on each axis in turn, the other
    axes and columns harmless; then the intensity edges of the variant."""
    imul = 65535.0 if variant == "lmc" else 1.0
    rng = np.random.default_rng(seed + 7)
    rnd, ties, edge = las_coords(seed, n, scale, off)
    v = np.concatenate([rnd, ties, edge])
    kind = np.concatenate([np.full(len(rnd), "random"), np.full(len(ties), "tie"), np.full(len(edge), "edge")])
    m = len(v)
    it = las_intensities(imul)
    rows = np.zeros((3 * m + len(it), 5))
    rows[:, :3] = off            # quotient 0 on the axes not under test
    for a in range(3):
        rows[a * m:(a + 1) * m, a] = v
    rows[:3 * m, 3] = rng.choice([0.0, 0.5, 1.0, 0.25], 3 * m) * (1.0 if variant == "lmc" else 65535.0)
    rows[3 * m:, 3] = it
    rows[:, 4] = rng.integers(0, 2 ** 37, len(rows))
    return rows, np.concatenate([kind, kind, kind, np.full(len(it), "intensity")])


def las_gps(seed, n):
    """-> (gps seconds off the nanosecond grid whose time fits int64, in frames of nearby times: list of
    arrays; times that do not: beyond 2^63 ns up to 2^40 s, the int64 edges on the refused side;
    the int64 edges on the accepted side, by sign)."""
    rng = np.random.default_rng(seed)
    frames = []
    per = max(n // 40, 8)
    for b in list(range(-6, 33)) + [33]:                 # frame bases 2^-6 .. 2^33 s (2^63 ns = 2^33.1 s)
        base = min(2.0 ** b, 9.2e9) * rng.uniform(1.0, 1.05)
        frames.append(base + np.sort(rng.uniform(0.0, 1.0, per)))
        if b % 5 == 0:
            frames.append(-base - rng.uniform(0.0, 1.0, per))
    e = 9223372036.854775807
    cand = _walk(np.array([e, -e]), 4)
    t = np.rint(cand * 1e9)
    fits = (t >= -2.0 ** 63) & (t < 2.0 ** 63)
    refused = np.concatenate([cand[~fits], 2.0 ** np.arange(34, 41) * 1.0000001, [-2.0 ** 40, 1e300, np.nan, INF, -INF]])
    return frames, refused, (cand[fits & (cand > 0)], cand[fits & (cand < 0)])
