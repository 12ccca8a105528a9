"""The batch's cache bookkeeping and the prep schedule (csrc/batch_state.hpp) compiled for the host with
g++ under ASan/UBSan, stand-alone: tests/host/batch_state_host.cpp drives scripted event sequences and
checks every decision against the rules written in the header.  No GPU, no library."""
import os

import pytest

import hostbuild
from hostbuild import CSRC

SCENARIOS = [
    "three_identical_calls",      # (prep, ordinary) / (prep, any-order, speculate) / hit: 2 preps for 3 calls
    "key_change_misses",          # each of the six key components, after a hit
    "work_in_flight_fences",
    "fence_after_each_launch",    # speculative: the next prep is ordinary; plain: it may be any-order
    "no_kernel",
    "pipelined_steps",            # n = 1, 2, 3 from either half
    "tuner",
    "forget_speculation",
    "batch_sums",
    "batch_spans_and_key",
    "batch_relative_table",
]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    exe = hostbuild.build(tmp_path_factory.mktemp("batch_state"), "batch_state_host.cpp", "-Wall", "-Werror", sanitize=True)
    return hostbuild.run(exe, timeout=60)


def test_every_scenario_ran_clean(host_run):
    assert host_run.returncode == 0, host_run.stderr[-3000:]
    assert host_run.stdout.split() == [w for s in SCENARIOS for w in ("ok", s)]


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(host_run, name):
    assert f"ok {name}\n" in host_run.stdout, host_run.stderr[-3000:]


def test_header_reads_no_hip():
    """The header is plain C++: what it includes is the standard library only."""
    with open(os.path.join(CSRC, "batch_state.hpp")) as f:
        inc = [line.split()[1] for line in f if line.startswith("#include")]
    assert inc and all(i.startswith("<") and "hip" not in i for i in inc), inc
