"""The evenly-timed rule of csrc/time_rule.hpp restated in NumPy, and the stored columns the CPU and GPU
tests share.

Frame f with n valid points is evenly timed when t_ns[i] == t0 + i * dt for every valid i, with
t0 = t_ns[0], dt = t_ns[1] - t_ns[0] (0 for n < 2), in int32 wrap-around arithmetic (uint32 modulo 2^32):
the arithmetic the deskew kernel generates a time in, so whatever the predicate accepts is reproduced to
the bit.  n = 0 is evenly timed.
"""
import numpy as np

I32_MAX = 2**31 - 1
I32_MIN = -2**31


def wrap32(v):
    """Python ints / int64 array -> the int32 they wrap to."""
    return (np.asarray(v, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def generate(t0, dt, n):
    i = np.arange(n, dtype=np.int64)
    return wrap32(int(t0) + i * int(dt))   # |i * dt| < 2^63 for every n a batch can hold


def rule_of(t):
    """(even, t0, dt) of one frame's stored int32 times."""
    t = np.asarray(t, dtype=np.int32)
    n = len(t)
    t0 = int(t[0]) if n > 0 else 0
    dt = int(wrap32(int(t[1]) - int(t[0]))) if n > 1 else 0
    return bool(np.array_equal(generate(t0, dt, n), t)), t0, dt


def ramp(t0, dt, n):
    """A ramp that stays inside int32 (asserted)."""
    v = int(t0) + np.arange(n, dtype=np.int64) * int(dt)
    assert n == 0 or (v.min() >= I32_MIN and v.max() <= I32_MAX)
    return v.astype(np.int32)


def synth_times(n):
    """k_synth's column: floor(i * 10^8 / n)."""
    return ((np.arange(n, dtype=np.int64) * 100_000_000) // max(n, 1)).astype(np.int32)


def off_by_one(t, i):
    t = np.array(t, dtype=np.int32)
    t[i] += 1
    return t


def host_cases():
    """name -> (stored times, expected even) for the host predicate."""
    big = 4100
    base = ramp(5, 1000, big)
    c = {
        "n0": (np.zeros(0, np.int32), True),
        "n1": (np.array([123], np.int32), True),
        "n2": (np.array([7, -9], np.int32), True),
        "dt0": (ramp(42, 0, 300), True),
        "dt_negative": (ramp(10_000_000, -2500, 3000), True),
        "dt1": (ramp(0, 1, 2049), True),
        "t0_negative": (ramp(-1_000_000, 1000, 1500), True),
        "reaches_int32_max": (ramp(I32_MAX - 999 * 1000, 1000, 1000), True),
        # i * dt leaves int32.  The declared arithmetic is wrap-around: a column that stores the WRAPPED
        # values is evenly timed (and generated back exactly); one that saturates instead is not.
        "wraps_stored_wrapped": (wrap32(np.arange(6, dtype=np.int64) * 2**30), True),
        "wraps_stored_saturated": (np.clip(np.arange(6, dtype=np.int64) * 2**30, I32_MIN, I32_MAX).astype(np.int32),
                                   False),
        "synth_n3": (synth_times(3), True),
        "synth_n7": (synth_times(7), False),
        "off_at_1": (off_by_one(base, 1), False),
        "off_at_last": (off_by_one(base, big - 1), False),
        "off_at_1024": (off_by_one(base, 1024), False),
        "off_at_2048": (off_by_one(base, 2048), False),
    }
    assert int(c["reaches_int32_max"][0][-1]) == I32_MAX
    assert int(c["synth_n7"][0][4]) == 57142857 and 4 * int(c["synth_n7"][0][1]) == 57142856
    return c
