"""The CSIM exports on the GPU (csim_export; csrc/csim_codecs.hpp): LivoxLVXWriter.write_lvx_file
(lvx / lvx2 / lvx3, CSIM:235-374) and DataExporter's PCD / XYZ / CSV (CSIM:1603-1715), byte for byte
against the reference's own files (tests/golden/csim_export.npz) and, on inputs the golden does not
hold, against the plain-Python statement of the formats (tests/csimexport.py, itself pinned to the
golden by test_csim_export_cpu.py)."""
import os
from ctypes import c_float, c_int64, c_uint8, c_uint64

import numpy as np
import pytest

import csimexport as CE
from conftest import golden

pytestmark = pytest.mark.gpu

VERSIONS = ("lvx", "lvx2", "lvx3")
FORMATS = ("pcd", "xyz", "csv")


@pytest.fixture(scope="module")
def g():
    return golden("csim_export.npz")


@pytest.fixture(scope="module")
def ex(mc):
    return mc.csim_export


def device_info(ex, g):
    return ex.DeviceInfo(str(g["dev_sn"]), int(g["dev_type"]), "03.08.0000", bool(g["dev_ext_enable"]),
                         *(float(v) for v in g["dev_ext"]))


def dev_dict(d):
    return dict(lidar_sn=d.lidar_sn, device_type=d.device_type, extrinsic_enable=d.extrinsic_enable, roll=d.roll,
                pitch=d.pitch, yaw=d.yaw, x=d.x, y=d.y, z=d.z)


def f_rows(g):
    return np.column_stack([g["F_xyz"], g["F_intensity"].astype(np.float64), g["F_timestamp"].astype(np.float64)])


def f_frames(mc, g):
    """Case F as the reference's frame dicts of LiDARPoint lists."""
    xyz, it, ts, tag = g["F_xyz"], g["F_intensity"], g["F_timestamp"], g["F_tag"]
    frames, i = [], 0
    for f, c in enumerate(g["F_counts"]):
        pts = [mc.LiDARPoint(float(xyz[j, 0]), float(xyz[j, 1]), float(xyz[j, 2]), int(it[j]), int(ts[j]), j % 4,
                             int(tag[j])) for j in range(i, i + int(c))]
        frames.append({"frame_id": f, "timestamp": int(g["F_frame_ts"][f]), "points": pts})
        i += int(c)
    return frames


def lvx_golden(g, version):
    return g["F_lvx" if version == "lvx" else "F_lvx2"].tobytes()


def check_case_f(mc, ctx, g):
    """Case F through the array encoders (also run after every error: the context stays usable)."""
    ex = mc.csim_export
    rows = f_rows(g)
    for version in VERSIONS:
        got = ex.encode_lvx(rows, g["F_counts"], g["F_frame_ts"], g["F_tag"], device_info(ex, g), version, ctx)
        assert got == lvx_golden(g, version), version
    for fmt, key in zip(FORMATS, ("F_pcd", "F_xyz_file", "F_csv")):
        head = {"pcd": ex.pcd_header(len(rows)), "xyz": b"", "csv": ex.CSV_HEADER}[fmt]
        assert head + ex.encode_text(rows, fmt, context=ctx) == g[key].tobytes(), fmt


# ---- 1. rows source against the golden ---------------------------------------------------------------
def test_rows_arrays_match_reference_files(mc, gpu_ctx, g, ex):
    check_case_f(mc, gpu_ctx, g)
    rows = f_rows(g)
    # per-frame clouds: the same lines, cut at the frame boundaries (empty frames give empty bodies)
    parts = ex.encode_text(rows, "pcd", counts=g["F_counts"], context=gpu_ctx)
    assert [len(p) == 0 for p in parts] == [c == 0 for c in g["F_counts"]]
    assert ex.pcd_header(len(rows)) + b"".join(parts) == g["F_pcd"].tobytes()
    # a wider row buffer (ld > 5) and no tags
    wide = np.column_stack([rows, np.full((len(rows), 2), np.nan)])
    got = ex.encode_lvx(wide, g["F_counts"], g["F_frame_ts"], None, device_info(ex, g), "lvx2", gpu_ctx)
    assert got == CE.lvx_bytes(rows, g["F_counts"], g["F_frame_ts"], None, dev_dict(device_info(ex, g)), "lvx2")
    assert ex.encode_text(wide, "csv", context=gpu_ctx) == CE.csv_body(rows)


@pytest.mark.parametrize("version", VERSIONS)
def test_write_lvx_file_matches_reference(mc, gpu_ctx, g, ex, version, tmp_path):
    p = tmp_path / f"f.{version}"
    ex.LivoxLVXWriter(version, context=gpu_ctx).write_lvx_file(str(p), f_frames(mc, g), device_info(ex, g))
    assert p.read_bytes() == lvx_golden(g, version)


def test_export_point_clouds_matches_reference(mc, gpu_ctx, g, ex, tmp_path):
    exporter = ex.DataExporter({}, context=gpu_ctx)
    exporter.export_point_clouds(f_frames(mc, g), str(tmp_path / "cloud"))
    assert sorted(os.listdir(tmp_path)) == ["cloud.csv", "cloud.pcd", "cloud.xyz"]       # no .las
    for ext, key in zip(FORMATS, ("F_pcd", "F_xyz_file", "F_csv")):
        assert (tmp_path / f"cloud.{ext}").read_bytes() == g[key].tobytes(), ext
    empty = tmp_path / "empty"
    empty.mkdir()
    exporter.export_point_clouds([{"timestamp": 0, "points": []}], str(empty / "cloud"))
    assert os.listdir(empty) == []


def test_text_edges_match_reference(gpu_ctx, g, ex, tmp_path):
    """Case T: NaN / inf / -0.0 in every column, "%.0f" ties, large values, a denormal, "%.6f" carries."""
    exporter = ex.DataExporter({}, context=gpu_ctx)
    rows = g["T_rows"]
    for fmt, fn in zip(FORMATS, (exporter._export_pcd, exporter._export_xyz, exporter._export_csv)):
        p = tmp_path / f"t.{fmt}"
        fn(rows, str(p))
        assert p.read_bytes() == g[f"T_{fmt}"].tobytes(), fmt
        assert ex.encode_text(rows, fmt, context=gpu_ctx) == CE.BODIES[fmt](rows)
    with pytest.raises(ValueError, match="2\\^107"):
        ex.encode_text(np.array([[1.0, 2.0, 3.0, 4.0, 2.0 ** 107]]), "pcd", context=gpu_ctx)
    assert ex.encode_text(np.array([[1.0, 2.0, 3.0, 4.0, 2.0 ** 107]]), "xyz", context=gpu_ctx) == b"1.000000 2.000000 3.000000\n"


# ---- 2. batch source ----------------------------------------------------------------------------------
def fill_batch(ctx, counts, xyz, intensity, starts, tags_seed=0):
    b = ctx.batch(counts, with_time=True)
    x, y, z = (np.ascontiguousarray(xyz[:, k], np.float32) for k in range(3))
    b.upload_columns(x, y, z, np.ascontiguousarray(intensity, np.float32))
    b.upload_time(np.concatenate([1000 * np.arange(c, dtype=np.int64) for c in counts] + [np.zeros(0, np.int64)]))
    b.set_frame_starts(starts)
    return b


def test_batch_source_matches_statement_and_rows_encoders(mc, gpu_ctx, g, ex):
    counts = g["F_counts"]
    # intensities with fractions (the row holds their truncation), 0 and 255.75
    it = g["F_intensity"].astype(np.float64) + np.where(np.arange(len(g["F_intensity"])) % 3 == 0, 0.75, 0.0)
    b = fill_batch(gpu_ctx, counts, g["F_xyz"], it, g["F_frame_ts"])
    rows = ex.batch_rows(b)
    assert rows.shape == (int(counts.sum()), 5) and rows[:, 3].max() == 255.0 and (rows[:, 3] == np.trunc(rows[:, 3])).all()
    assert np.array_equal(rows[:, 0], g["F_xyz"][:, 0].astype(np.float32).astype(np.float64))
    assert np.array_equal(rows[:, 4], (np.repeat(g["F_frame_ts"], counts)
                                       + np.concatenate([1000 * np.arange(c) for c in counts])).astype(np.float64))
    dev = device_info(ex, g)
    tags = g["F_tag"].astype(np.uint8)
    for version in VERSIONS:
        got = ex.encode_lvx_batch(b, dev, version, tags=tags)
        assert got == CE.lvx_bytes(rows, counts, g["F_frame_ts"], tags, dev_dict(dev), version), version
        assert got == ex.encode_lvx(rows, counts, g["F_frame_ts"], tags, dev, version, gpu_ctx), version
    assert ex.encode_lvx_batch(b, dev, "lvx2") == CE.lvx_bytes(rows, counts, g["F_frame_ts"], None, dev_dict(dev), "lvx2")
    for fmt in FORMATS:
        got = ex.encode_text_batch(b, fmt)
        assert b"".join(got) == CE.BODIES[fmt](rows), fmt
        assert got == ex.encode_text(rows, fmt, counts=counts, context=gpu_ctx), fmt
    b.close()


def test_batch_without_time_or_starts_is_a_state_error(mc, gpu_ctx, g, ex):
    lib, ptr = gpu_ctx.lib, mc._lib.ptr
    dev = device_info(ex, g)
    sn, dtype, ext_on, ext = ex._device_fields(dev)
    ts = np.zeros(2, np.uint64)
    pos = np.zeros(3, np.int64)
    out = gpu_ctx.device_buffer(4096)
    for b in (gpu_ctx.batch([3, 2]), gpu_ctx.batch([3, 2], with_time=True)):    # no time; time but no frame starts
        rc = lib.mc_csim_lvx_encode_batch(gpu_ctx.handle, 2, b.handle, ptr(ts, c_uint64), None, ptr(sn, c_uint8), dtype,
                                          ext_on, ptr(ext, c_float), out.ptr, 4096)
        assert rc == mc._lib.MC_ERR_STATE
        rc = lib.mc_csim_text_encode_batch(gpu_ctx.handle, 0, b.handle, out.ptr, 4096, ptr(pos, c_int64))
        assert rc == mc._lib.MC_ERR_STATE
        with pytest.raises(mc.McError, match="-4"):
            ex.encode_text_batch(b, "pcd")
        with pytest.raises((mc.McError, ValueError)):
            ex.encode_lvx_batch(b, dev, "lvx2")
        b.close()
    out.close()
    check_case_f(mc, gpu_ctx, g)


# ---- 3. the MC_ERR_SPACE protocol of the text encoders ----------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_text_space_protocol(mc, gpu_ctx, g, ex, fmt):
    lib, ptr = gpu_ctx.lib, mc._lib.ptr
    rows = f_rows(g)
    counts = np.ascontiguousarray(g["F_counts"], np.int64)
    want = CE.BODIES[fmt](rows)
    total, guard = len(want), 64
    d_rows = gpu_ctx.device_buffer(rows.nbytes)
    d_rows.from_host(rows)
    buf = gpu_ctx.device_buffer(total + guard)
    buf.from_host(np.full(total + guard, 0xAB, np.uint8))
    pos = np.zeros(len(counts) + 1, np.int64)
    code = ex.FORMATS[fmt]
    try:
        rc = lib.mc_csim_text_encode(gpu_ctx.handle, code, d_rows.ptr, 5, len(counts), ptr(counts, c_int64), buf.ptr,
                                     total - 1, ptr(pos, c_int64))
        assert rc == mc._lib.MC_ERR_SPACE
        assert int(pos[-1]) == total and pos[0] == 0 and (np.diff(pos) >= 0).all()
        line = [len(l) + 1 for l in want.split(b"\n")[:-1]]
        assert pos.tolist() == np.concatenate([[0], np.cumsum(line)])[np.concatenate([[0], np.cumsum(counts)])].tolist()
        assert (buf.to_host(np.uint8) == 0xAB).all()                     # nothing written
        rc = lib.mc_csim_text_encode(gpu_ctx.handle, code, d_rows.ptr, 5, len(counts), ptr(counts, c_int64), None, 0,
                                     ptr(pos, c_int64))
        assert rc == mc._lib.MC_ERR_SPACE and int(pos[-1]) == total      # sizes only
        rc = lib.mc_csim_text_encode(gpu_ctx.handle, code, d_rows.ptr, 5, len(counts), ptr(counts, c_int64), buf.ptr,
                                     total, ptr(pos, c_int64))
        assert rc == 0
        back = buf.to_host(np.uint8)
        assert back[:total].tobytes() == want
        assert (back[total:] == 0xAB).all()                              # the guard bytes stay
    finally:
        buf.close()
        d_rows.close()


def test_lvx_space_and_guard(mc, gpu_ctx, g, ex):
    lib, ptr = gpu_ctx.lib, mc._lib.ptr
    rows = f_rows(g)
    counts = np.ascontiguousarray(g["F_counts"], np.int64)
    ts = np.ascontiguousarray(g["F_frame_ts"], np.uint64)
    sn, dtype, ext_on, ext = ex._device_fields(device_info(ex, g))
    d_rows = gpu_ctx.device_buffer(rows.nbytes)
    d_rows.from_host(rows)
    for version in (1, 2):
        want = lvx_golden(g, "lvx" if version == 1 else "lvx2")
        buf = gpu_ctx.device_buffer(len(want) + 64)
        buf.from_host(np.full(len(want) + 64, 0xAB, np.uint8))
        args = (gpu_ctx.handle, version, d_rows.ptr, 5, len(counts), ptr(counts, c_int64), ptr(ts, c_uint64), None,
                ptr(sn, c_uint8), dtype, ext_on, ptr(ext, c_float), buf.ptr)
        assert lib.mc_csim_lvx_encode(*args, len(want) - 1) == mc._lib.MC_ERR_SPACE
        assert (buf.to_host(np.uint8) == 0xAB).all()
        assert lib.mc_csim_lvx_encode(*args, len(want)) == 0
        back = buf.to_host(np.uint8)
        assert (back[len(want):] == 0xAB).all()
        dev = dev_dict(device_info(ex, g))
        assert back[:len(want)].tobytes() == CE.lvx_bytes(rows, counts, ts, None, dev, "lvx" if version == 1 else "lvx2")
        buf.close()
    d_rows.close()


# ---- 4. where the reference's write raises -----------------------------------------------------------
ERROR_POINTS = [("lvx2", (float("nan"), 1.0, 1.0)), ("lvx2", (1.0, float("inf"), 1.0)), ("lvx2", (1.0, 1.0, float("-inf"))),
                ("lvx3", (float("nan"), 1.0, 1.0)), ("lvx2", (2147483.65, 1.0, 1.0)), ("lvx2", (1.0, -2147483.66, 1.0)),
                ("lvx2", (1.0, 1.0, 1e300)), ("lvx", (3.5e38, 1.0, 1.0)), ("lvx", (1.0, -1e39, 1.0)),
                ("lvx", (1.0, 1.0, 3.4028235677973366e38))]   # the last: the tie between FLT_MAX and 2^128 rounds up


@pytest.mark.parametrize("version,xyz", ERROR_POINTS)
def test_write_errors_raise_before_the_file_exists(mc, gpu_ctx, g, ex, version, xyz, tmp_path):
    frames = f_frames(mc, g)[3:6]
    frames[1]["points"][200] = mc.LiDARPoint(*xyz, 7, 5, 0, 0)
    p = tmp_path / f"bad.{version}"
    with pytest.raises(ValueError):
        ex.LivoxLVXWriter(version, context=gpu_ctx).write_lvx_file(str(p), frames, device_info(ex, g))
    assert os.listdir(tmp_path) == []
    rows, counts, ts, tags = ex.frames_to_rows(frames)
    with pytest.raises(ValueError):       # the plain statement agrees
        CE.lvx_bytes(rows, counts, ts, tags, dev_dict(device_info(ex, g)), version)
    check_case_f(mc, gpu_ctx, g)


def test_intensity_errors_and_edges_that_pack(mc, gpu_ctx, g, ex, tmp_path):
    dev = device_info(ex, g)
    base = f_rows(g)[:300].copy()
    counts, ts = [100, 200], [5, 6]
    for version in ("lvx", "lvx2"):
        for v in (float("nan"), 256.0, -1.0, float("inf"), 1e30):
            rows = base.copy()
            rows[257, 3] = v
            with pytest.raises(ValueError):
                ex.encode_lvx(rows, counts, ts, None, dev, version, gpu_ctx)
            with pytest.raises(ValueError):
                CE.lvx_bytes(rows, counts, ts, None, dev_dict(dev), version)
    # a LiDARPoint whose intensity / tag is not an int in 0..255 never reaches the device
    frames = f_frames(mc, g)[3:5]
    frames[1]["points"][0] = mc.LiDARPoint(1.0, 2.0, 3.0, 300, 5, 0, 0)
    with pytest.raises(ValueError, match="int in 0..255"):
        ex.LivoxLVXWriter("lvx2", context=gpu_ctx).write_lvx_file(str(tmp_path / "bad.lvx2"), frames, dev)
    assert os.listdir(tmp_path) == []
    # what does not raise: fractions truncate toward zero (255.9 -> 255, -0.9 -> 0), the largest int32
    # products, NaN and infinities packed as float32 by the legacy writer, float32 denormals and the
    # largest finite float32
    rows = base.copy()
    rows[0, 3], rows[1, 3], rows[2, 3] = 255.9, -0.9, 0.5
    rows[3, :3] = [2147483.647, -2147483.648, 2147483.6474]
    assert ex.encode_lvx(rows, counts, ts, None, dev, "lvx2", gpu_ctx) == CE.lvx_bytes(rows, counts, ts, None, dev_dict(dev), "lvx2")
    rows[3, :3] = [float("nan"), float("inf"), float("-inf")]
    rows[4, :3] = [1e-40, -1e-45, 7e-46]
    rows[5, :3] = [3.4028234e38, -3.4028235e38, 3.40282356779733e38]   # the last: just below the tie that overflows
    assert ex.encode_lvx(rows, counts, ts, None, dev, "lvx", gpu_ctx) == CE.lvx_bytes(rows, counts, ts, None, dev_dict(dev), "lvx")
    check_case_f(mc, gpu_ctx, g)


# ---- 5. many workgroups per frame, many frames per launch -------------------------------------------
def test_forty_frames_of_five_thousand_points_both_sources(mc, gpu_ctx, g, ex):
    rng = np.random.default_rng(404)
    F, n = 40, 5000
    counts = np.full(F, n, np.int64)
    xyz = rng.uniform(-95.0, 95.0, (F * n, 3))
    xyz[rng.integers(0, F * n, 500), rng.integers(0, 3, 500)] = rng.integers(-12000, 12000, 500) / 128.0   # "%.6f" ties
    it = rng.uniform(0.0, 255.99, F * n)
    starts = np.array([int((1.7e9 + 0.1 * f) * 1e9) for f in range(F)], np.int64)
    tags = rng.integers(0, 2, F * n).astype(np.uint8)
    b = fill_batch(gpu_ctx, counts, xyz, it, starts)
    rows = ex.batch_rows(b)                     # float32-valued rows: one reference serves both sources
    dev = device_info(ex, g)
    for version in ("lvx", "lvx2"):
        want = CE.lvx_bytes(rows, counts, starts, tags, dev_dict(dev), version)
        assert ex.encode_lvx_batch(b, dev, version, tags=tags) == want, version
        assert ex.encode_lvx(rows, counts, starts, tags, dev, version, gpu_ctx) == want, version
    for fmt in FORMATS:
        want = CE.BODIES[fmt](rows)
        assert b"".join(ex.encode_text_batch(b, fmt)) == want, fmt
        assert ex.encode_text(rows, fmt, context=gpu_ctx) == want, fmt
    b.close()
    # full float64 rows (not float32 values) through the rows source
    rows64 = np.column_stack([xyz, np.trunc(it), rows[:, 4]])
    assert ex.encode_lvx(rows64, counts, starts, tags, dev, "lvx2", gpu_ctx) == \
        CE.lvx_bytes(rows64, counts, starts, tags, dev_dict(dev), "lvx2")
    assert ex.encode_text(rows64, "pcd", context=gpu_ctx) == CE.pcd_body(rows64)
