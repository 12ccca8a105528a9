"""The host walk over LVX files (csrc/ingest_index.cpp behind mc_lvx_probe / mc_lvx_index; f7): the
three golden byte strings — LVX v1.1 (tests/golden/codecs.npz, LMC:57-272), CSIM legacy lvx and lvx2
(tests/golden/csim_export.npz, CSIM:256-374; lvx3 is lvx2's bytes) — against the numpy walk of
tests/ingest.py, the malformed files every decode must refuse before a launch, and the same walker
as a stand-alone program under ASan + UBSan.  No GPU: both entry points are host only."""
import ctypes
import os
import shutil
import struct
from ctypes import c_float, c_int, c_int32, c_int64, c_uint8, c_uint64

import numpy as np
import pytest

import hostbuild
import ingest as ING
from conftest import golden, pkg


def files():
    c, e = golden("codecs.npz"), golden("csim_export.npz")
    assert bool(e["F_lvx3_is_lvx2"])
    return {"v11": c["lvx/bytes"].tobytes(), "lvx": e["F_lvx"].tobytes(), "lvx2": e["F_lvx2"].tobytes(),
            "lvx3": e["F_lvx2"].tobytes()}


def malformed():
    """name -> bytes, each a golden with bytes edited."""
    f = files()
    v11, leg, l2 = f["v11"], f["lvx"], f["lvx2"]
    w = ING.lvx_walk(v11)
    p4, p5 = int(w["frame_pos"][4]), int(w["frame_pos"][5])
    put = lambda b, at, fmt, v: b[:at] + struct.pack(fmt, v) + b[at + struct.calcsize(fmt):]   # noqa: E731
    w2 = ING.lvx_walk(l2)
    q9 = int(w2["frame_pos"][9])
    out = {
        "v11 cut mid-record": v11[:-5],
        "v11 cut mid-frame-header": v11[:p5 + 10],
        "v11 cut inside the file header": v11[:50],
        "v11 next offset backwards": put(v11, p4 + 8, "<Q", p4 - 24),
        "v11 next offset to itself": put(v11, p4 + 8, "<Q", p4),
        "v11 next offset past the end": put(v11, p4 + 8, "<Q", len(v11) + 1366),
        "v11 next offset off the package multiple": put(v11, p4 + 8, "<Q", p5 + 2),
        "v11 wrong magic": put(v11, 20, "<I", 0xAC0EA768),
        "lvx2 cut mid-record": l2[:-3],
        "lvx2 cut mid-frame-header": l2[:q9 + 20],
        "lvx2 cut inside the file header": l2[:30],
        "lvx2 count beyond the file": put(l2, q9 + 12, "<I", 769 + 4000),
        "lvx2 count 2^32 - 1": put(l2, q9 + 12, "<I", 0xFFFFFFFF),
        "lvx2 wrong magic": put(l2, 16, "<I", 0),
        "legacy cut mid-record": leg[:-1],
        "legacy cut inside the file header": leg[:40],
        "legacy count beyond the file": put(leg, int(ING.lvx_walk(leg)["frame_pos"][9]) + 8, "<I", 1 << 30),
        "legacy frame count in the header": put(leg, 14, "<I", 13),
        "unknown signature": b"livox_data" + v11[10:],
        "unknown version": v11[:16] + bytes([1, 2, 0, 0]) + v11[20:],
        "zero length": b"",
    }
    return out


def probe(lib, data):
    raw = np.frombuffer(data, np.uint8)
    fmt, nf = c_int(-7), c_int32(-7)
    rc = lib.mc_lvx_probe(raw.ctypes.data_as(ctypes.c_void_p) if len(raw) else None, len(raw), ctypes.byref(fmt),
                          ctypes.byref(nf))
    return rc, fmt.value, nf.value


def index(lib, data, fmt, F):
    raw = np.frombuffer(data, np.uint8)
    pos, slots = np.full(F + 1, -1, np.int64), np.full(F, -1, np.int64)
    ids, ts = np.zeros(F, np.uint64), np.zeros(F, np.int64)
    sn, dt, ee, ext = np.zeros(16, np.uint8), c_uint8(), c_uint8(), np.zeros(6, np.float32)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))   # noqa: E731
    rc = lib.mc_lvx_index(raw.ctypes.data_as(ctypes.c_void_p), len(raw), fmt, F, P(pos, c_int64), P(slots, c_int64),
                          P(ids, c_uint64), P(ts, c_int64), P(sn, c_uint8), ctypes.byref(dt), ctypes.byref(ee),
                          P(ext, c_float))
    return rc, pos, slots, ids, ts, (sn.tobytes().split(b"\x00")[0].decode(), dt.value, bool(ee.value), ext)


@pytest.mark.parametrize("name", ["v11", "lvx", "lvx2", "lvx3"])
def test_index_equals_the_numpy_walk(name):
    lib = pkg()._lib.load()
    data = files()[name]
    w = ING.lvx_walk(data)
    rc, fmt, F = probe(lib, data)
    assert rc == 0, lib.mc_last_error()
    assert fmt == {"v11": 0, "lvx": 1, "lvx2": 2, "lvx3": 2}[name] == w["format"]
    assert F == len(w["slots"])
    rc, pos, slots, ids, ts, dev = index(lib, data, fmt, F)
    assert rc == 0, lib.mc_last_error()
    assert np.array_equal(pos, w["frame_pos"]) and pos[-1] == len(data)
    assert np.array_equal(slots, w["slots"])
    assert np.array_equal(ids, w["ids"])
    assert np.array_equal(ts, w["ts"])
    sn, ty, en, ext = ING.device_block(data)
    assert dev[:3] == (sn, ty, en) and np.array_equal(dev[3], ext)
    if name == "v11":
        c = golden("codecs.npz")
        assert slots.tolist() == [192, 0, 96, 96, 384, 1056]
        assert ids.tolist() == [int(c[f"lvx/{i}/frame_id"]) for i in range(6)]
        assert ts.tolist() == [int(float(c[f"lvx/{i}/timestamp"]) * 1e9) if slots[i] else -1 for i in range(6)]
        assert [ING.lvx_trimmed(r) for r in w["recs"]] == [97, 0, 96, 1, 300, 1000]
    else:
        e = golden("csim_export.npz")
        assert slots.tolist() == [0, 1, 0, 2, 255, 256, 257, 767, 768, 769, 3, 0] == e["F_counts"].tolist()
        assert np.array_equal(ts, e["F_frame_ts"])
        assert ids.tolist() == list(range(12))
        assert dev[0] == str(e["dev_sn"]) and dev[1] == int(e["dev_type"])
        if name != "lvx":   # the legacy header stores neither the flag nor the extrinsics
            assert dev[2] == bool(e["dev_ext_enable"])
            assert np.array_equal(dev[3], e["dev_ext"].astype(np.float32))


@pytest.mark.parametrize("name", sorted(malformed()))
def test_malformed_file_is_refused_with_a_message(name):
    lib = pkg()._lib.load()
    rc, fmt, F = probe(lib, malformed()[name])
    assert rc == pkg()._lib.MC_ERR_INVALID
    assert (fmt, F) == (-7, -7)   # nothing reported for a refused file
    assert len(lib.mc_last_error()) > 10


def test_index_refuses_another_format_or_frame_count():
    lib = pkg()._lib.load()
    data = files()["lvx2"]
    assert index(lib, data, 1, 12)[0] == pkg()._lib.MC_ERR_INVALID
    assert index(lib, data, 2, 11)[0] == pkg()._lib.MC_ERR_INVALID
    assert index(lib, data, 2, 13)[0] == pkg()._lib.MC_ERR_INVALID


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_walker_stand_alone_under_asan_ubsan(tmp_path):
    exe = hostbuild.build(tmp_path, "ingest_index_host.cpp", os.path.join(hostbuild.CSRC, "ingest_index.cpp"), sanitize=True)
    paths, want = [], []
    for i, (name, data) in enumerate(list(files().items()) + sorted(malformed().items())):
        p = tmp_path / f"case_{i:02d}.bin"
        p.write_bytes(data)
        paths.append(str(p))
        want.append(name in files())
    r = hostbuild.run(exe, *paths)
    assert "contradictions 0" in r.stdout
    lines = {ln.split(" ", 1)[0]: ln.split(" ")[1] for ln in r.stdout.splitlines() if ln.startswith(str(tmp_path))}
    for p, ok in zip(paths, want):
        assert lines[p] == ("ok" if ok else "invalid"), (p, lines[p])
