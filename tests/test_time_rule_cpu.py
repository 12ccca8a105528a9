"""The evenly-timed rule (csrc/time_rule.hpp) compiled for the host with g++, stand-alone, against the
NumPy restatement of tests/timerule.py.  No GPU.

The rule's one arithmetic is int32 wrap-around: the predicate compares a stored time with what the
deskew kernel generates for its index, so "evenly timed" means "generated back to the bit"."""
import struct

import numpy as np
import pytest

import hostbuild
import timerule as TR


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    """Every host case through the compiled core, once: name -> (even, t0, dt, generated times)."""
    d = tmp_path_factory.mktemp("time_rule")
    exe = hostbuild.build(d, "time_rule_host.cpp", "-Wall", "-Werror")
    cases = TR.host_cases()
    src, dst = d / "in.bin", d / "out.bin"
    blob = struct.pack("<q", len(cases))
    for t, _ in cases.values():
        blob += struct.pack("<q", len(t)) + np.ascontiguousarray(t, np.int32).tobytes()
    src.write_bytes(blob)
    hostbuild.run(exe, src, dst, timeout=60)
    out = np.frombuffer(dst.read_bytes(), np.int32)
    res, k = {}, 0
    for name, (t, _) in cases.items():
        n = len(t)
        res[name] = (int(out[k]), int(out[k + 1]), int(out[k + 2]), out[k + 3:k + 3 + n])
        k += 3 + n
    assert k == len(out)
    return res


@pytest.mark.parametrize("name", list(TR.host_cases()))
def test_predicate_matches_numpy(host_results, name):
    t, want_even = TR.host_cases()[name]
    even, t0, dt, gen = host_results[name]
    n_even, n_t0, n_dt = TR.rule_of(t)
    assert n_even == want_even, "the NumPy restatement disagrees with the case's stated decision"
    assert (bool(even), t0, dt) == (n_even, n_t0, n_dt)
    # generation is the predicate's other side: it equals the NumPy ramp always, the stored column
    # exactly when the frame is evenly timed
    assert np.array_equal(gen, TR.generate(n_t0, n_dt, len(t)))
    assert np.array_equal(gen, t) == want_even


def test_wrap_decision(host_results):
    """A column whose i * dt leaves int32: the core's declared arithmetic (wrap-around) accepts the
    column that stores the wrapped values and generates it back; the saturated one is refused."""
    t, _ = TR.host_cases()["wraps_stored_wrapped"]
    assert list(t[:4]) == [0, 2**30, -2**31, -2**30]
    even, t0, dt, gen = host_results["wraps_stored_wrapped"]
    assert (even, t0, dt) == (1, 0, 2**30) and np.array_equal(gen, t)
    assert host_results["wraps_stored_saturated"][0] == 0


def test_near_misses_name_the_index():
    """The restatement itself: one point 1 ns off is found wherever it sits."""
    base = TR.ramp(5, 1000, 4100)
    assert TR.rule_of(base)[0]
    for i in (1, 1024, 2048, 4099):
        assert not TR.rule_of(TR.off_by_one(base, i))[0]
    assert TR.rule_of(TR.off_by_one(base[:2], 1)) == (True, 5, 1001)   # two points are always a ramp
