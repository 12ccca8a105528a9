"""The device text formatters behind the CSIM exports (DataExporter._export_pcd / _xyz / _csv,
CSIM:1643-1715) compiled for the host with g++ and checked against the C library's correctly rounded
formatting: the kernel's own source — the "%.6f" formatter of fmt6_core.hpp and the "%.0f" formatter and
line-descriptor prepare / emit of csim_text_core.hpp — included by tests/host/csim_text_host.cpp and
exercised on this CPU (no GPU): random doubles over every exponent up to 2^107, the planted "%.0f" and
"%.6f" ties, +-0, NaN / inf, and whole PCD / XYZ / CSV lines."""
import shutil

import pytest

import hostbuild


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_text_formatters_match_printf(tmp_path):
    r = hostbuild.run(hostbuild.build(tmp_path, "csim_text_host.cpp"), 200000, timeout=120)
    assert "bad 0" in r.stdout
