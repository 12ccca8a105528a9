"""The per-record cores of the LAS kernels (csrc/las_core.hpp: las_encode_rec, las_decode_rec,
las_time_ns) compiled for the host with g++ and
compared bit for bit with the numpy restatement of tests/las.py — the kernel's own source included
by tests/host/las_host.cpp and run on this CPU (no GPU).  Encode: the rounding ties, both int32 edges
+-1 ulp of the quotient, -0.0, denormals, NaN and +-inf (flagged), intensities at both ends.  Decode:
20 000 random full-range int32 X at scale 0.001 / offset 500000.0, where a fused multiply-add changes
the result of over 1 000 rows (counted exactly with fractions.Fraction) — and a mutant of the harness
that fuses them must fail the comparison."""
import shutil

import numpy as np
import pytest

import hostbuild
import las as LAS

UNFUSED = "  return p + off;\n"
FUSED = "  return fma((double)X, scale, off);\n"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """The harness, and the harness as the compiler reads it with las_unscale's two roundings fused."""
    tmp = tmp_path_factory.mktemp("las_host")
    text = hostbuild.preprocessed("las_host.cpp", "-ffp-contract=off")
    assert text.count(UNFUSED) == 1
    mutant = tmp / "las_host_fma.ii"
    mutant.write_text(text.replace(UNFUSED, FUSED))
    return tmp, hostbuild.build(tmp, "las_host.cpp", "-ffp-contract=off"), hostbuild.build(tmp, mutant, "-ffp-contract=off")


def run(exe, tmp, mode, head, body):
    src, dst = tmp / "in.bin", tmp / "out.bin"
    src.write_bytes(head + body)
    hostbuild.run(exe, mode, src, dst, timeout=120)
    return dst.read_bytes()


ENC_OUT = np.dtype([("X", "<i4", (3,)), ("intensity", "<u4"), ("gps", "<f8"), ("bad", "<i4"), ("zero", "<i4")])


def encode_cases():
    """(scale, offset, imul, tmul, rows (N, 5))"""
    na, inf = np.nan, np.inf
    tie = [0.005, 0.015, 0.025, -0.005, -0.015, 21474836.47, 21474836.48, -21474836.485, -21474836.49, 0.0, -0.0]
    e = 2147483647.5    # scale 1: the quotient is the coordinate
    edge = [e, np.nextafter(e, 0), np.nextafter(e, inf), -e - 1.0, np.nextafter(-e - 1.0, 0), np.nextafter(-e - 1.0, -inf),
            -0.5, 0.5, 1.5, 2.5, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, na, inf, -inf, 1e300, -1e300]
    rng = np.random.default_rng(2)
    out = []
    for scale, off, vals in ((0.01, 0.0, tie), (1.0, 0.0, edge), (0.001, 500000.0, list(rng.uniform(-1.6e6, 2.6e6, 4000))),
                             (0.01, -3.25, list(rng.uniform(-2.2e7, 2.2e7, 4000)))):
        v = np.array(vals)
        n = len(v)
        rows = np.zeros((3 * n, 5))
        for k in range(3):   # each value on each axis, the other axes harmless
            rows[k * n:(k + 1) * n, k] = v
        rows[:, 3] = rng.choice([0.0, 0.5, 1.0, 0.9999999, 1e-5, 0.25], 3 * n)
        rows[:, 4] = rng.integers(0, 2 ** 37, 3 * n)
        out.append((scale, off, 65535.0, 0.0, rows))
        out.append((scale, off, 1.0, 1e-9, rows * np.array([1, 1, 1, 65535.0, 1])))
    it = np.array([0.0, -0.0, -0.5, -0.9999999, -1.0, 65535.0, 65535.9999, 65536.0, 1e30, -1e30, na, inf, -inf, 5e-324, 255.5])
    rows = np.zeros((len(it), 5))
    rows[:, 3] = it
    rows[:, 4] = [na, inf, -inf] + [2.0 ** 62] * (len(it) - 3)
    out.append((0.01, 0.0, 1.0, 1e-9, rows))
    out.append((0.01, 0.0, 65535.0, 0.0, rows))   # tmul 0: gps 0.0 whatever column 4 holds
    return out


def test_encode_core_equals_the_restatement(exes):
    tmp, exe, _ = exes
    flagged = accepted = 0
    for scale, off, imul, tmul, rows in encode_cases():
        head = np.array([scale] * 3 + [off] * 3 + [imul, tmul]).tobytes()
        got = np.frombuffer(run(exe, tmp, "enc", head, np.ascontiguousarray(rows).tobytes()), ENC_OUT)
        assert len(got) == len(rows)
        bad = np.zeros(len(rows), bool)
        for k in range(3):
            X, b = LAS.fix(rows[:, k], scale, off)
            assert np.array_equal(got["X"][:, k], X), (scale, off, k)
            bad |= b
        it, b = LAS.intensity(rows[:, 3], imul)
        bad |= b
        assert np.array_equal(got["intensity"], it)
        assert np.array_equal(got["bad"] != 0, bad)
        gps = rows[:, 4] * tmul if tmul != 0.0 else np.zeros(len(rows))
        assert np.array_equal(LAS.bits(got["gps"]), LAS.bits(gps))
        flagged += int(bad.sum())
        accepted += int((~bad).sum())
    assert flagged >= 30 and accepted >= 40000
    # the named edges, on their own
    X, b = LAS.fix(np.array([2147483647.5, np.nextafter(2147483647.5, 0), -2147483648.5, np.nextafter(-2147483648.5, -np.inf)]), 1.0, 0.0)
    assert b.tolist() == [True, False, False, True] and X[1:3].tolist() == [2147483647, -2147483648]


def decode_input(fmt, reclen, scale, off, X, gps):
    rec = np.zeros(len(X), LAS.RECORD[fmt])
    rec["X"], rec["Y"], rec["Z"] = X, X[::-1], np.roll(X, 7)
    rec["intensity"] = np.arange(len(X)) * 13 % 65536
    if fmt & 1:
        rec["gps_time"] = gps
    wide = np.full((len(X), reclen), LAS.PAD, np.uint8)
    wide[:, :LAS.NOMINAL[fmt]] = np.frombuffer(rec.tobytes(), np.uint8).reshape(len(X), -1)
    head = np.array([fmt, reclen], np.int64).tobytes() + np.array([scale] * 3 + [off] * 3).tobytes()
    return rec, head, wide.tobytes()


DEC_OUT = np.dtype([("v", "<f8", (5,)), ("t", "<i8"), ("fits", "<i8")])


def test_decode_core_equals_the_restatement_and_a_fused_mutant_does_not(exes):
    tmp, exe, mutant = exes
    rng = np.random.default_rng(1)
    X = rng.integers(-2 ** 31, 2 ** 31, 20000)
    X[:4] = [-2 ** 31, 2 ** 31 - 1, 0, -1]
    assert LAS.fused_differs(X, 0.001, 500000.0) >= 1000
    ts = rng.integers(0, 2 ** 37, 20000)
    gps = ts * 1e-9
    gps[:6] = [np.nan, np.inf, -np.inf, 1e300, -0.0, 9.2e9]
    for fmt, reclen in ((3, 34), (1, 30), (0, 20), (2, 28)):
        rec, head, body = decode_input(fmt, reclen, 0.001, 500000.0, X, gps)
        got = np.frombuffer(run(exe, tmp, "dec", head, body), DEC_OUT)
        want = np.stack([LAS.unscale(rec[n], 0.001, 500000.0) for n in "XYZ"], 1)
        assert np.array_equal(LAS.bits(got["v"][:, :3]), LAS.bits(want)), fmt
        assert np.array_equal(got["v"][:, 3], rec["intensity"])
        g = rec["gps_time"] if fmt & 1 else np.zeros(len(X))
        assert np.array_equal(LAS.bits(got["v"][:, 4]), LAS.bits(g))
        t, ok = LAS.time_ns(g)
        assert np.array_equal(got["fits"] != 0, ok) and np.array_equal(got["t"][ok], t[ok])
        if fmt == 3:
            assert not ok[:4].any() and ok[4:].all()
            assert np.array_equal(got["t"][6:], ts[6:])   # rint((ts * 1e-9) * 1e9) == ts below 2^37 ns
            bad = np.frombuffer(run(mutant, tmp, "dec", head, body), DEC_OUT)
            differ = (LAS.bits(bad["v"][:, :3]) != LAS.bits(want)).any(axis=1)
            assert differ.sum() >= 1000   # the comparison above fails for the fused harness
    # scale with offset 0 shows nothing: both harnesses agree there
    rec, head, body = decode_input(3, 34, 0.001, 0.0, X, gps)
    a = np.frombuffer(run(exe, tmp, "dec", head, body), DEC_OUT)
    b = np.frombuffer(run(mutant, tmp, "dec", head, body), DEC_OUT)
    assert np.array_equal(LAS.bits(a["v"][:, :3]), LAS.bits(b["v"][:, :3]))
