"""CPU sanitizer builds: the library's host-side code compiled with g++ under
AddressSanitizer + UndefinedBehaviorSanitizer and exercised here, no GPU needed.

* ``plan_host``: the batch layout / tile builder (``plan_batch``, behind ``mc_batch_create``) and
  the merged-cloud gather plan + its finishing copies (``plan_gather`` / ``gather_finish``, behind
  ``mc_comm_gather_batch`` and ``mc_gather_batches``) — ``csrc/plan.cpp`` itself, with host memcpy
  in place of the device copies and the RCCL receives; worlds 1-8, empty shards, 4/5-column
  shards, every root.
* ``pcd_formatter_host``: the device ``%.6f`` line writers (pcd_line_core.hpp), as in
  ``test_pcd_formatter_host.py``, now under the sanitizers.
* ``devbuf_host``: the owning device buffer (``csrc/devbuf.hpp``) with malloc / free behind its
  allocation seam: growth, injected allocation failures, moves, partial construction, and the live
  account that ``mc_device_memory_live`` reports; leaks are errors.
"""
import os
import re
import shutil

import pytest

import hostbuild

ROOT = hostbuild.ROOT

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@needs_gxx
def test_plan_host_under_asan_ubsan(tmp_path):
    exe = hostbuild.build(tmp_path, "plan_host.cpp", os.path.join(hostbuild.CSRC, "plan.cpp"), sanitize=True)
    assert "bad 0" in hostbuild.run(exe).stdout


@needs_gxx
def test_pcd_formatter_under_asan_ubsan(tmp_path):
    exe = hostbuild.build(tmp_path, "pcd_formatter_host.cpp", sanitize=True)
    assert "bad 0" in hostbuild.run(exe, 50000).stdout


@needs_gxx
def test_devbuf_host_under_asan_ubsan(tmp_path):
    exe = hostbuild.build(tmp_path, "devbuf_host.cpp", "-DMC_DEVBUF_HOST_TEST", sanitize=True)
    assert "bad 0" in hostbuild.run(exe).stdout


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
