"""The CSIM export formats without a GPU: tests/csimexport.py (the plain-Python statement of the five
formats) pinned byte for byte to the reference's own files (tests/golden/csim_export.npz, cases F and
T), the host-only mc_csim_lvx_layout against it, and the argument validation of
csim_export (LivoxLVXWriter.write_lvx_file CSIM:235-374, DataExporter CSIM:1603-1715)."""
import numpy as np
import pytest

import csimexport as CE
from conftest import golden, pkg


@pytest.fixture(scope="module")
def g():
    return golden("csim_export.npz")


def case_f(g):
    rows = np.column_stack([g["F_xyz"], g["F_intensity"].astype(np.float64), g["F_timestamp"].astype(np.float64)])
    dev = dict(lidar_sn=str(g["dev_sn"]), device_type=int(g["dev_type"]), extrinsic_enable=bool(g["dev_ext_enable"]),
               **dict(zip(("roll", "pitch", "yaw", "x", "y", "z"), (float(v) for v in g["dev_ext"]))))
    return rows, g["F_counts"], g["F_frame_ts"], g["F_tag"].astype(np.uint8), dev


def test_golden_case_f_shape(g):
    assert g["F_counts"].tolist() == [0, 1, 0, 2, 255, 256, 257, 767, 768, 769, 3, 0]
    assert bool(g["F_lvx3_is_lvx2"])
    xyz = g["F_xyz"]
    assert np.signbit(xyz[xyz == 0.0]).any() and (~np.signbit(xyz[xyz == 0.0])).any()
    assert (xyz == -0.9999).any() and {0, 255} <= set(g["F_intensity"].tolist()) and set(g["F_tag"].tolist()) == {0, 1}
    # frame starts and unit starts of the lvx2 file fall on odd byte offsets
    pos = CE.lvx_layout(g["F_counts"], "lvx2")
    assert (pos[:-1] % 2 == 1).any() and (pos[:-1] % 2 == 0).any()


@pytest.mark.parametrize("version", ["lvx", "lvx2", "lvx3"])
def test_statement_lvx_matches_reference(g, version):
    rows, counts, fts, tags, dev = case_f(g)
    want = g["F_lvx" if version == "lvx" else "F_lvx2"].tobytes()
    got = CE.lvx_bytes(rows, counts, fts, tags, dev, version)
    assert got == want
    assert CE.lvx_layout(counts, version)[-1] == len(want)


@pytest.mark.parametrize("fmt,key", [("pcd", "F_pcd"), ("xyz", "F_xyz_file"), ("csv", "F_csv"),
                                     ("pcd", "T_pcd"), ("xyz", "T_xyz"), ("csv", "T_csv")])
def test_statement_text_matches_reference(g, fmt, key):
    rows = case_f(g)[0] if key.startswith("F") else g["T_rows"]
    assert CE.text_file(rows, fmt) == g[key].tobytes()


def test_lvx2_truncates_toward_zero_and_has_21_byte_package_header(g):
    rows, counts, fts, tags, dev = case_f(g)
    b = g["F_lvx2"].tobytes()
    pos = CE.lvx_layout(counts, "lvx2")
    i, col = (int(v[0]) for v in np.nonzero(rows[:, :3] == -0.9999))
    f = int(np.searchsorted(np.cumsum(counts), i, side="right"))
    at = int(pos[f]) + 45 + 14 * (i - int(np.cumsum(counts)[f - 1])) + 4 * col
    assert int.from_bytes(b[at:at + 4], "little", signed=True) == -999
    assert b[int(pos[1]) + 24:int(pos[1]) + 34] == bytes([5, 0, 1, 0, 0, 0, 0, 0, 1, 2])
    assert int(pos[1]) - int(pos[0]) == 45    # an empty frame is its 24 + 21 header bytes


def test_statement_raises_where_the_reference_does():
    dev = dict(lidar_sn="A", device_type=1, extrinsic_enable=False, roll=0, pitch=0, yaw=0, x=0, y=0, z=0)
    ok = [1.0, 2.0, 3.0, 7.0, 0.0]
    for version, col, v in [("lvx2", 0, np.nan), ("lvx2", 1, np.inf), ("lvx2", 2, 2147483.648), ("lvx2", 0, -2147483.649),
                            ("lvx", 0, 3.5e38), ("lvx", 3, 256.0), ("lvx2", 3, -1.0), ("lvx2", 3, np.nan)]:
        r = list(ok)
        r[col] = v
        with pytest.raises(ValueError):
            CE.lvx_bytes(np.array([r]), [1], [0], None, dev, version)
    # the edges that do not raise: the largest products, a NaN / inf packed as float32, intensity 255.9
    CE.lvx_bytes(np.array([[2147483.647, -2147483.648, 0.0, 255.9, 0.0]]), [1], [0], None, dev, "lvx2")
    CE.lvx_bytes(np.array([[np.nan, np.inf, -np.inf, 0.0, 0.0]]), [1], [0], None, dev, "lvx")


@pytest.mark.parametrize("version", ["lvx", "lvx2", "lvx3"])
def test_layout_matches_statement(version):
    ex = pkg().csim_export
    rng = np.random.default_rng(5)
    for counts in ([], [0], [0, 1, 0, 2, 255, 256, 257, 767, 768, 769, 3, 0], rng.integers(0, 5000, 40).tolist()):
        assert ex.lvx_layout(counts, version).tolist() == CE.lvx_layout(counts, version).tolist()


def test_layout_rejects_bad_arguments():
    m = pkg()
    lib = m._lib.load()
    counts = np.array([1, -2], np.int64)
    pos = np.zeros(3, np.int64)
    rc = lib.mc_csim_lvx_layout(2, 2, m._lib.ptr(counts, m._lib.c_int64), m._lib.ptr(pos, m._lib.c_int64))
    assert rc == m._lib.MC_ERR_INVALID
    assert lib.mc_csim_lvx_layout(4, 0, None, m._lib.ptr(pos, m._lib.c_int64)) == m._lib.MC_ERR_INVALID
    with pytest.raises(ValueError, match="Unsupported format version: lvx4"):
        m.csim_export.lvx_layout([1], "lvx4")


def test_argument_validation_raises_as_specified():
    m = pkg()
    ex = m.csim_export
    with pytest.raises(ValueError, match="^Unsupported format version: lvx4$"):
        ex.LivoxLVXWriter("lvx4")
    assert ex.LivoxLVXWriter().format_version == "lvx2"
    assert m.LivoxLVXWriter is m.codecs.LivoxLVXWriter       # the top-level name stays the LMC writer
    assert m.DataExporter is ex.DataExporter and m.DeviceInfo is ex.DeviceInfo
    P = m.LiDARPoint
    good = P(1.0, 2.0, 3.0, 7, 1000, 0, 1)
    for bad in (P(1.0, 2.0, 3.0, 256, 0, 0, 0), P(1.0, 2.0, 3.0, -1, 0, 0, 0), P(1.0, 2.0, 3.0, 7.0, 0, 0, 0),
                P(1.0, 2.0, 3.0, 7, 0, 0, 256), P(1.0, 2.0, 3.0, 7, 0, 0, -1), P(1.0, 2.0, 3.0, 7, 0, 0, 0.5)):
        with pytest.raises(ValueError, match="int in 0..255"):
            ex.frames_to_rows([{"timestamp": 5, "points": [good, bad]}])
    with pytest.raises(ValueError, match="u64"):
        ex.frames_to_rows([{"timestamp": -1, "points": [good]}])
    rows, counts, ts, tags = ex.frames_to_rows([{"timestamp": 5, "points": []}, {"timestamp": 2 ** 64 - 1, "points": [good]}])
    assert rows.tolist() == [[1.0, 2.0, 3.0, 7.0, 1000.0]] and counts.tolist() == [0, 1]
    assert ts.tolist() == [5, 2 ** 64 - 1] and tags.tolist() == [1]
    dev = ex.DeviceInfo("SN", 1, "fw", True, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="Unsupported text format"):
        ex.encode_text(np.zeros((1, 5)), "las")
    with pytest.raises(IndexError):
        ex.encode_text(np.zeros((1, 4)), "pcd")
    with pytest.raises(ValueError, match="add up"):
        ex.encode_text(np.zeros((3, 5)), "pcd", counts=[1, 1])
    with pytest.raises(ValueError, match="Unsupported format version"):
        ex.encode_lvx(np.zeros((1, 5)), [1], [0], None, dev, "lvx4")
    with pytest.raises(ValueError, match="one timestamp per frame"):
        ex.encode_lvx(np.zeros((1, 5)), [1], [0, 1], None, dev, "lvx2")
    with pytest.raises(ValueError, match="one tag per row"):
        ex.encode_lvx(np.zeros((1, 5)), [1], [0], np.zeros(2, np.uint8), dev, "lvx2")
    with pytest.raises(ValueError, match="16 bytes"):
        ex.encode_lvx(np.zeros((1, 5)), [1], [0], None, ex.DeviceInfo("S" * 17, 1, "", False, 0, 0, 0, 0, 0, 0), "lvx2")
    with pytest.raises(ValueError):
        ex.encode_lvx(np.zeros((1, 5)), [1], [0], None, ex.DeviceInfo("SN", 300, "", False, 0, 0, 0, 0, 0, 0), "lvx2")
    assert ex.pcd_header(3) == CE.PCD_HEADER.format(n=3).encode() and ex.CSV_HEADER == CE.CSV_HEADER.encode()
