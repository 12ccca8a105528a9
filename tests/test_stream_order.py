"""The codec kernels' unit order (unit_order.hpp stream_unit, DESIGN §4 "Codec unit order"): the
header compiled for the host with g++ (tests/host/stream_order_host.cpp), checked to be a bijection on [0, n) for every
order and n, and to start where the order it answers ended (reversed: the last unit first; XCD
ranges reversed: each of xcd_unit<true>'s 8 ranges from its tail)."""
import shutil

import pytest

import hostbuild


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_stream_unit_is_a_bijection_starting_at_the_hot_end(tmp_path):
    r = hostbuild.run(hostbuild.build(tmp_path, "stream_order_host.cpp"), timeout=120)
    assert "bad 0" in r.stdout, r.stdout[-2000:]
