"""The device text-token parser behind the ingest decoders (read_points / read_points_batch, the
inverse of LMC:932-948 and CSIM:1643-1715) compiled for the host with g++ and compared bit for bit
with the C library's correctly rounded strtod: the kernel's own source — the token-parser section of
csrc/ingest.hpp — spliced into tests/host/ingest_host.cpp and exercised on this CPU (no GPU): over
200 k random in-window tokens covering every significant-digit count 1..19 with every fractional
length 0..19, the planted integers around 2^53 / 2^63 / 2^64 with and without a fraction, decimal ties,
-0.000000, leading zeros, "5.", nan / inf / -inf, the empty CSV field; out-of-window tokens (20 digits,
an exponent, "1.2.3", "--1", "abc") must be flagged and carry no value."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livox-motion-compensation-sim_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host", "ingest_host.cpp")


def token_section() -> str:
    src = open(os.path.join(CSRC, "ingest.hpp")).read()
    return src[src.index("struct IngestTok {"):src.index("// (end of the token parser section")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_token_parser_matches_strtod(tmp_path):
    code = open(HARNESS).read().replace("// TOKEN_SECTION", token_section())
    cpp = tmp_path / "ingest_host.cpp"
    cpp.write_text(code)
    exe = tmp_path / "ingest_host"
    r = subprocess.run(["g++", "-O2", "-std=c++17", str(cpp), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "530"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "bad 0" in r.stdout
    checked = int(r.stdout.split("checked ")[1].split()[0])
    assert checked >= 4 * 200_000   # each token with four kinds of ending
