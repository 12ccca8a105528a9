"""Every core header (DESIGN.md "Core headers") compiles on its own for the host: a translation unit of two
lines, the stand-ins of tests/host/device_standins.hpp and then the header, through
g++ -std=c++17 -fsyntax-only -Wall -Werror.  A core that starts to lean on its device header, or on a builtin
without a stand-in, fails here before a harness has to find out."""
import shutil
import subprocess

import pytest

import hostbuild


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("header", hostbuild.CORE_HEADERS)
def test_core_header_is_self_contained(tmp_path, header):
    tu = tmp_path / "tu.cpp"
    tu.write_text(f'#include "device_standins.hpp"\n#include "{header}"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", hostbuild.CSRC, "-I", hostbuild.HOST,
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
