"""The host parser of a LAS public header block (csrc/las_index.cpp behind mc_las_probe; f8) against
the files of the numpy restatement (tests/las.py): formats 0..3, offsets to point data 227 and 243,
record lengths nominal and nominal + 2; the malformed files every decode must refuse before a launch;
and the same parser as a stand-alone program under ASan + UBSan.  No GPU: the entry point is host only."""
import ctypes
import os
import shutil
import struct
from ctypes import c_double, c_int32, c_int64

import numpy as np
import pytest

import hostbuild
import las as LAS
from conftest import pkg


def rows(n=37, seed=4):
    rng = np.random.default_rng(seed)
    r = np.empty((n, 5))
    r[:, :3] = rng.uniform(-900, 900, (n, 3))
    r[:, 3] = rng.integers(0, 256, n)
    r[:, 4] = 1_000_000_000 + 1000 * np.arange(n)
    return r


def files():
    out = {}
    for fmt in range(4):
        for at in (227, 243):
            for extra in (0, 2):
                out[f"f{fmt} at {at} +{extra}"] = LAS.encode(rows(), "csim", 0.001, [500000.0, -3.0, 0.0], fmt,
                                                             reclen=LAS.NOMINAL[fmt] + extra, offset_to_points=at)
    unit = rows() / np.array([1, 1, 1, 255.0, 1])   # save_las takes intensities in 0..1
    out["empty cloud"] = LAS.encode(rows(0), "lmc")
    out["version 1.0"] = LAS.encode(unit, "lmc", minor=0)
    out["version 1.3"] = LAS.encode(unit, "lmc", minor=3)
    return out


def malformed():
    good = LAS.encode(rows(), "csim")
    put = lambda at, fmt, v: good[:at] + struct.pack(fmt, v) + good[at + struct.calcsize(fmt):]   # noqa: E731
    return {
        "wrong signature": b"LASX" + good[4:],
        "version 1.4": put(25, "B", 4),
        "version 2.0": good[:24] + bytes([2, 0]) + good[26:],
        "format 4": put(104, "B", 4),
        "format 3 with the LAZ bit": put(104, "B", 0x83),
        "header cut at 100 bytes": good[:100],
        "header cut at 226 bytes": good[:226],
        "header size 226": put(94, "<H", 226),
        "offset below the header size": put(94, "<H", 300),
        "offset past the end": put(96, "<I", len(good) + 1),
        "record length below nominal": put(105, "<H", 33),
        "count x record length past the end": put(107, "<I", 38),
        "count 2^32 - 1": put(107, "<I", 0xFFFFFFFF),
        "file cut mid-record": good[:-1],
        "zero length": b"",
        "three bytes": b"LAS",
    }


def probe(lib, data):
    raw = np.frombuffer(data, np.uint8)
    fmt, rl, off, n = c_int32(-7), c_int32(-7), c_int64(-7), c_int64(-7)
    s, o, b = np.full(3, -7.0), np.full(3, -7.0), np.full(6, -7.0)
    P = lambda a: a.ctypes.data_as(ctypes.POINTER(c_double))   # noqa: E731
    rc = lib.mc_las_probe(raw.ctypes.data_as(ctypes.c_void_p) if len(raw) else None, len(raw), ctypes.byref(fmt),
                          ctypes.byref(rl), ctypes.byref(off), ctypes.byref(n), P(s), P(o), P(b))
    return rc, (fmt.value, rl.value, off.value, n.value), s, o, b


@pytest.mark.parametrize("name", sorted(files()))
def test_probe_equals_the_restatement(name):
    lib = pkg()._lib.load()
    data = files()[name]
    h = LAS.parse_header(data)
    rc, (fmt, rl, off, n), s, o, b = probe(lib, data)
    assert rc == 0, lib.mc_last_error()
    assert (fmt, rl, off, n) == (int(h["format"]), int(h["reclen"]), int(h["offset_to_points"]), int(h["count"]))
    assert np.array_equal(s, h["scale"]) and np.array_equal(o, h["offset"]) and np.array_equal(b, h["bounds"])
    if name.startswith("f"):
        f, at, extra = int(name[1]), int(name.split()[2]), int(name.split("+")[1])
        assert (fmt, rl, off, n) == (f, LAS.NOMINAL[f] + extra, at, 37)
        assert len(data) == at + 37 * rl
        # the records are checked against the file size: one byte short is refused
        assert probe(lib, data[:-1])[0] == pkg()._lib.MC_ERR_INVALID


@pytest.mark.parametrize("name", sorted(malformed()))
def test_malformed_header_is_refused_with_a_message(name):
    lib = pkg()._lib.load()
    rc, got, s, o, b = probe(lib, malformed()[name])
    assert rc == pkg()._lib.MC_ERR_INVALID
    assert got == (-7, -7, -7, -7) and (s == -7.0).all() and (b == -7.0).all()   # nothing reported for a refused file
    assert len(lib.mc_last_error()) > 10
    with pytest.raises(ValueError):
        pkg().las._probe(malformed()[name])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_parser_stand_alone_under_asan_ubsan(tmp_path):
    exe = hostbuild.build(tmp_path, "las_index_host.cpp", os.path.join(hostbuild.CSRC, "las_index.cpp"), sanitize=True)
    paths, want = [], []
    for i, (name, data) in enumerate(sorted(files().items()) + sorted(malformed().items())):
        p = tmp_path / f"case_{i:02d}.bin"
        p.write_bytes(data)
        paths.append(str(p))
        want.append(name in files())
    r = hostbuild.run(exe, *paths)
    assert "contradictions 0" in r.stdout
    lines = {ln.split(" ", 1)[0]: ln.split(" ")[1] for ln in r.stdout.splitlines() if ln.startswith(str(tmp_path))}
    for p, ok in zip(paths, want):
        assert lines[p] == ("ok" if ok else "invalid"), (p, lines[p])
