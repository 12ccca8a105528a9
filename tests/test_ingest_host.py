"""The device text-token parser behind the ingest decoders (read_points / read_points_batch, the
inverse of LMC:932-948 and CSIM:1643-1715) compiled for the host with g++ and compared bit for bit
with the C library's correctly rounded strtod: the kernel's own source — the token parser of
csrc/ingest_token_core.hpp — included by tests/host/ingest_host.cpp and exercised on this CPU (no GPU): over
200 k random in-window tokens covering every significant-digit count 1..19 with every fractional
length 0..19, the planted integers around 2^53 / 2^63 / 2^64 with and without a fraction, decimal ties,
-0.000000, leading zeros, "5.", nan / inf / -inf, the empty CSV field; out-of-window tokens (20 digits,
an exponent, "1.2.3", "--1", "abc") must be flagged and carry no value."""
import shutil

import pytest

import hostbuild


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_token_parser_matches_strtod(tmp_path):
    r = hostbuild.run(hostbuild.build(tmp_path, "ingest_host.cpp"), 530, timeout=120)
    assert "bad 0" in r.stdout
    checked = int(r.stdout.split("checked ")[1].split()[0])
    assert checked >= 4 * 200_000   # each token with four kinds of ending
