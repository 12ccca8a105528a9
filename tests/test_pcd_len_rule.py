"""The packed ASCII-PCD text-length rule the summing kernels use (layout.hpp PcdCount), checked on
the CPU against "%.6f" (LMC:948's format) for float32 values around every boundary where the length
changes, plus a log-uniform sample: a value's text is 9 + [sign bit] + [|v| >= 10] + [|v| >= 100] +
[|v| >= 1000] bytes (separator included), each test a compare of the float's upper 16 bits, and every
value the rule does not cover (NaN, inf, |v| >= 4288) is flagged slow, which sends its block to the
measure pass and the exact formatter.  The constants are read from layout.hpp, so the test follows
the kernel source."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "livox-motion-compensation-sim_amd", "csrc", "layout.hpp")
CODECS = os.path.join(ROOT, "livox-motion-compensation-sim_amd", "csrc", "pcd_line_core.hpp")


def _constants():
    src = open(LAYOUT).read()
    body = src[src.index("struct PcdCount"):]
    thresholds = [int(h, 16) & 0xFFFF for h in re.findall(r"pk_gt_u16\(m, (0x[0-9A-Fa-f]{8})u\)", body)]
    slow = int(re.search(r"kPcdSlowBits = (0x[0-9A-Fa-f]{8})u", src).group(1), 16) >> 16
    return thresholds, slow


def _rule(v):
    """(bytes, slow) per float32 value, as PcdCount computes them (upper halves, sign bit)."""
    h = (np.asarray(v, np.float32).view(np.uint32) >> 16).astype(np.int64)
    m = h & 0x7FFF
    thresholds, slow = _constants()
    n = 9 + (h >> 15)
    for c in thresholds:
        n = n + (m > c)
    return n, m >= slow


def _printf_len(v):
    return np.array([len("%.6f" % float(x)) + 1 for x in v], np.int64)


def _around(b, k=2048):
    """the k float32 values on each side of b (and of -b)"""
    c = np.float32(b).view(np.int32)
    pos = np.arange(c - k, c + k + 1, dtype=np.int32).view(np.float32)
    return np.concatenate([pos, -pos])


def test_rule_constants_are_the_decades():
    thresholds, slow = _constants()
    assert thresholds == [0x411F, 0x42C7, 0x4479]
    for c, t in zip(thresholds, (10.0, 100.0, 1000.0)):
        # T's low half is zero, so |v| >= T <=> upper(|v|) > upper(T) - 1
        assert np.float32(t).view(np.uint32) == (c + 1) << 16
    assert np.float32(4288.0).view(np.uint32) == slow << 16


def test_rule_matches_printf_at_every_boundary():
    vals = np.concatenate([_around(b) for b in (1e-7, 5e-7, 1e-6, 0.1, 1.0, 9.9999995, 10.0, 99.99999, 100.0,
                                                999.9999, 1000.0, 4286.0)]
                          + [np.array([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38], np.float32)])
    n, slow = _rule(vals)
    assert not slow.any()
    assert np.array_equal(n, _printf_len(vals))


def test_rule_matches_printf_on_a_log_uniform_sample():
    rng = np.random.default_rng(11)
    mag = np.exp(rng.uniform(np.log(1e-9), np.log(4287.9), 200_000)).astype(np.float32)
    vals = mag * rng.choice(np.array([-1, 1], np.float32), mag.size)
    n, slow = _rule(vals)
    assert not slow.any()
    assert np.array_equal(n, _printf_len(vals))


def test_everything_off_the_packed_formatter_is_slow():
    """The packed writer takes |v| < 4294 (pcd_line_core.hpp); the rule flags from 4288 on, NaN and inf
    included, so no value the packed writer cannot format keeps a block off the measure pass."""
    assert "fabsf(v) < 4294.0f" in open(CODECS).read()
    edge = _around(4288.0, 64)
    n, slow = _rule(edge)
    assert np.array_equal(slow, np.abs(edge) >= 4288.0)
    big = np.array([4294.0, 4294.967, 1e4, 3.4e38, np.inf, -np.inf, np.nan, -np.nan], np.float32)
    assert _rule(big)[1].all()
    # below the slow mark every value is one the packed writer formats
    below = _around(4288.0, 64)
    below = below[np.abs(below) < 4288.0]
    assert (np.abs(below) < 4294.0).all() and not _rule(below)[1].any()
