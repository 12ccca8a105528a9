"""CPU sanitizer builds: the library's host-side code compiled with g++ under
AddressSanitizer + UndefinedBehaviorSanitizer and exercised here, no GPU needed.

* ``plan_host``: the batch layout / tile builder (``plan_batch``, behind ``mc_batch_create``) and
  the merged-cloud gather plan + its finishing copies (``plan_gather`` / ``gather_finish``, behind
  ``mc_comm_gather_batch`` and ``mc_gather_batches``) — ``csrc/plan.cpp`` itself, with host memcpy
  in place of the device copies and the RCCL receives; worlds 1-8, empty shards, 4/5-column
  shards, every root.
* ``pcd_formatter_host``: the device ``%.6f`` line writers (codecs.hpp), as in
  ``test_pcd_formatter_host.py``, now under the sanitizers.
* ``devbuf_host``: the owning device buffer (``csrc/devbuf.hpp``) with malloc / free behind its
  allocation seam: growth, injected allocation failures, moves, partial construction, and the live
  account that ``mc_device_memory_live`` reports; leaks are errors.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livox-motion-compensation-sim_amd", "csrc")
SAN = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@needs_gxx
def test_plan_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "plan_host"
    subprocess.run(["g++", *SAN, f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "plan_host.cpp"),
                    os.path.join(CSRC, "plan.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "bad 0" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


@needs_gxx
def test_pcd_formatter_under_asan_ubsan(tmp_path):
    from test_pcd_formatter_host import HARNESS, formatter_section
    code = open(HARNESS).read().replace("// FORMATTER_SECTION", formatter_section())
    cpp = tmp_path / "fmt.cpp"
    cpp.write_text(code)
    exe = tmp_path / "fmt"
    subprocess.run(["g++", *SAN, str(cpp), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), "50000"], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "bad 0" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-3000:]


@needs_gxx
def test_devbuf_host_under_asan_ubsan(tmp_path):
    exe = tmp_path / "devbuf_host"
    subprocess.run(["g++", *SAN, "-DMC_DEVBUF_HOST_TEST", f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "devbuf_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "bad 0" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_device_memory_live_exported_and_abi_unchanged():
    from conftest import pkg
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    name = "mc_device_memory_live"
    assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name)
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # no context, so nothing of the library's is allocated; either output may be NULL
    b, k = m._lib.c_int64(-1), m._lib.c_int64(-1)
    assert lib.mc_device_memory_live(m._lib.ctypes.byref(b), m._lib.ctypes.byref(k)) == m._lib.MC_OK
    assert b.value >= 0 and k.value >= 0
    assert lib.mc_device_memory_live(None, None) == m._lib.MC_OK
