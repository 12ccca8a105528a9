"""Whose intensity column a batch holds (csrc/batch_state.hpp: intensity_copied_from / holds_intensity_of /
points_version) compiled for the host with g++ under ASan/UBSan, stand-alone:
tests/host/keep_intensity_host.cpp drives the events of deskews and of the other writers and checks every
answer against the rule written in the header.  No GPU, no library."""
import pytest

import hostbuild

SCENARIOS = [
    "held_after_the_event",
    "own_write_then_event_holds_again",   # and: a launch that failed to queue claims nothing
    "output_written",                     # points_written() on the output; other events change nothing
    "input_written",
    "another_uid",                        # another source, a new batch, uid 0
    "stale_source_version",
    "in_place_needs_no_state",
    "many_versions",
]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    exe = hostbuild.build(tmp_path_factory.mktemp("keep_intensity"), "keep_intensity_host.cpp", "-Wall", "-Werror", sanitize=True)
    return hostbuild.run(exe, timeout=60)


def test_every_scenario_ran_clean(host_run):
    assert host_run.returncode == 0, host_run.stderr[-3000:]
    assert host_run.stdout.split() == [w for s in SCENARIOS for w in ("ok", s)]


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(host_run, name):
    assert f"ok {name}\n" in host_run.stdout, host_run.stderr[-3000:]
