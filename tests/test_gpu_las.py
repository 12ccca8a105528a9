"""LAS 1.2 on the GPU (las.py; csrc/las.hpp, f8): files written from device rows and from a batch, byte
for byte against the numpy restatement of tests/las.py; the refusals; files decoded into rows bit for
bit and into a batch; the round trip into a deskew and the two opt-in hooks.  Every output of the
C-ABI calls sits between 256-byte guards of 0xA5 that must survive."""
import contextlib
import ctypes
import io
import json
import os
from ctypes import c_double, c_int64

import numpy as np
import pytest

import las as LAS
from conftest import GOLDEN, golden
from test_gpu_csim_export import f_frames, f_rows
from test_gpu_ingest import guarded, inner, open_guard
from test_gpu_run import digests, log_lines
from test_gpu_scan import CFGS, restore_rng, traj_of

pytestmark = pytest.mark.gpu

T = 512      # k_las_encode: records per workgroup
TD = 256     # k_las_decode
DATE = (2024, 61)
SIZES = [0, 1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 3]


@pytest.fixture(scope="module")
def software(mc):
    assert mc.las.TILE_RECORDS == T and mc.las.DECODE_TILE_RECORDS == TD
    return f"mcdeskew {mc.__version__}".encode()


def make_rows(n, variant, seed=0, ld=5):
    rng = np.random.default_rng(seed + n)
    r = np.full((n, ld), np.nan)   # columns past the fifth are never read
    r[:, :3] = rng.uniform(-2000, 2000, (n, 3))
    k = rng.random((n, 3)) < 0.2
    r[:, :3][k] = np.round(r[:, :3][k] * 200) / 200 + 0.0025 * rng.integers(0, 2, int(k.sum()))   # ties at both scales
    r[:, 3] = rng.random(n) if variant == "lmc" else rng.integers(0, 65536, n) + rng.choice([0.0, 0.5, 0.99], n)
    if variant == "lmc" and n:
        r[:3, 3] = [1.0, 0.0, 0.9999999][:n]
    if ld > 4:
        r[:, 4] = rng.integers(0, 2 ** 37, n)
    return r


def encode_rows_guarded(mc, ctx, rows, variant, fmt, software, scale=None, offset=None):
    """mc_las_encode into a guarded buffer -> (rc, file bytes, bad row)."""
    imul, tmul, dscale = LAS.VARIANTS[variant]
    s, o = LAS.xyz3(scale, dscale), LAS.xyz3(offset, 0.0)
    n, ld = rows.shape
    size = 227 + n * LAS.NOMINAL[fmt]
    d_rows = ctx.device_buffer(max(rows.nbytes, 8))
    if rows.size:
        d_rows.from_host(rows)
    out = guarded(ctx, size)
    bad = c_int64(-9)
    P = mc._lib.ptr
    rc = ctx.lib.mc_las_encode(ctx.handle, d_rows.ptr, ld, n, fmt, P(s, c_double), P(o, c_double), imul, tmul, software,
                               DATE[0], DATE[1], inner(out), size, ctypes.byref(bad))
    d_rows.close()
    return rc, open_guard(out, size).tobytes(), bad.value


def encode_batch_guarded(mc, ctx, batch, variant, fmt, software, scale=None, offset=None):
    imul, tmul, dscale = LAS.VARIANTS[variant]
    s, o = LAS.xyz3(scale, dscale), LAS.xyz3(offset, 0.0)
    size = 227 + batch.n_points * LAS.NOMINAL[fmt]
    out = guarded(ctx, size)
    bad = c_int64(-9)
    P = mc._lib.ptr
    rc = ctx.lib.mc_las_encode_batch(ctx.handle, batch.handle, fmt, P(s, c_double), P(o, c_double), imul, tmul, software,
                                     DATE[0], DATE[1], inner(out), size, ctypes.byref(bad))
    return rc, open_guard(out, size).tobytes(), bad.value


def check_bounds(data):
    h = LAS.parse_header(data)
    fmt, n = int(h["format"]), int(h["count"])
    rec = np.frombuffer(data, LAS.RECORD[fmt], n, 227)
    for k, name in enumerate("XYZ"):
        want = [LAS.unscale(rec[name].max(), h["scale"][k], h["offset"][k]),
                LAS.unscale(rec[name].min(), h["scale"][k], h["offset"][k])] if n else [0.0, 0.0]
        assert h["bounds"][2 * k:2 * k + 2].tolist() == want, name


# ---- 4. encode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_encode_rows(mc, gpu_ctx, software, n):
    for variant, lds in (("lmc", (4, 5, 7)), ("csim", (5, 7))):
        for ld in lds:
            rows = make_rows(n, variant, ld=ld)
            for fmt, scale, offset in ((3, None, None), (1, None, None), (3, [0.001, 0.01, 0.5], [500000.0, -3.25, 0.0])):
                want = LAS.encode(rows[:, :min(ld, 5)] if ld >= 5 else np.column_stack([rows, np.zeros(n)]), variant, scale,
                                  offset, fmt, software, *DATE)
                rc, got, bad = encode_rows_guarded(mc, gpu_ctx, rows, variant, fmt, software, scale, offset)
                assert rc == 0 and bad == -1, gpu_ctx.lib.mc_last_error()
                assert got == want, (variant, ld, fmt, scale)
                check_bounds(got)
    # formats 0 and 2, and the module function (today's date apart)
    rows = make_rows(n, "csim")
    for fmt in (0, 2):
        rc, got, _ = encode_rows_guarded(mc, gpu_ctx, rows, "csim", fmt, software)
        assert rc == 0 and got == LAS.encode(rows, "csim", fmt=fmt, software=software, year=DATE[0], day=DATE[1])
    assert mc.encode_las(rows, "csim", creation_date=DATE, context=gpu_ctx) == LAS.encode(rows, "csim", software=software,
                                                                                          year=DATE[0], day=DATE[1])


def make_batch(ctx, counts, variant, seed=1):
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    r = make_rows(n, variant, seed)
    cols = [np.ascontiguousarray(r[:, k], np.float32) for k in range(4)]
    if variant == "csim":
        cols[3] = np.minimum(cols[3], np.float32(65535.5))
    rng = np.random.default_rng(seed)
    t = rng.integers(-5_000_000, 100_000_000, n).astype(np.int32)
    starts = 1_000_000_000 + 100_000_000 * np.arange(len(counts), dtype=np.int64)
    b = ctx.batch(counts, with_time=True)
    b.upload_columns(*cols)
    b.upload_time(t)
    b.set_frame_starts(starts)
    return b, LAS.batch_rows(cols, t, counts, starts)


@pytest.mark.parametrize("n", SIZES)
def test_encode_batch(mc, gpu_ctx, software, n):
    counts = [0, 0, n // 3, 0, n - n // 3, 0]   # empty frames first, between and last
    for variant in ("lmc", "csim"):
        b, rows = make_batch(gpu_ctx, counts, variant)
        for fmt in (3, 1):
            rc, got, bad = encode_batch_guarded(mc, gpu_ctx, b, variant, fmt, software)
            assert rc == 0 and bad == -1, gpu_ctx.lib.mc_last_error()
            assert got == LAS.encode(rows, variant, fmt=fmt, software=software, year=DATE[0], day=DATE[1]), (variant, fmt)
            check_bounds(got)
        assert mc.encode_las(b, variant, creation_date=DATE) == LAS.encode(rows, variant, software=software, year=DATE[0],
                                                                           day=DATE[1])
    # a batch without a time column: the lmc variant needs none, the csim variant refuses
    plain = gpu_ctx.batch([n])
    r = make_rows(n, "lmc")
    cols = [np.ascontiguousarray(r[:, k], np.float32) for k in range(4)]
    plain.upload_columns(*cols)
    rc, got, _ = encode_batch_guarded(mc, gpu_ctx, plain, "lmc", 3, software)
    assert rc == 0 and got == LAS.encode(LAS.batch_rows(cols, None, [n], None, False), "lmc", software=software,
                                         year=DATE[0], day=DATE[1])
    with pytest.raises(ValueError, match="time column"):
        mc.encode_las(plain, "csim")
    assert encode_batch_guarded(mc, gpu_ctx, plain, "csim", 3, software)[0] == mc._lib.MC_ERR_STATE


# ---- 5. refusals -------------------------------------------------------------------------------------------
BAD = [(0, np.nan), (1, np.inf), (2, -np.inf), (0, 21474836.48), (1, -21474836.49), (3, np.nan), (3, 1.00002), (3, -2e-5)]


@pytest.mark.parametrize("where", ["first", "tile", "last"])
def test_refusals_name_the_row(mc, gpu_ctx, software, where, tmp_path):
    n = 2 * T + 3
    at = {"first": 0, "tile": T, "last": n - 1}[where]
    there = tmp_path / "there.las"
    there.write_bytes(b"earlier content")
    for col, v in BAD:
        rows = make_rows(n, "lmc", ld=4)
        rows[at, col] = v
        rc, _, bad = encode_rows_guarded(mc, gpu_ctx, rows, "lmc", 3, software)   # open_guard: the guards survived
        assert rc == mc._lib.MC_ERR_INVALID and bad == at, (col, v)
        with pytest.raises(ValueError, match=rf"row {at} \(the first of 1\)"):
            mc.write_las(there, rows, context=gpu_ctx)
        with pytest.raises(ValueError, match=rf"row {at} "):
            mc.write_las(tmp_path / "new.las", rows, context=gpu_ctx)
        assert there.read_bytes() == b"earlier content" and not (tmp_path / "new.las").exists()
    # two refused rows: the first is named; from a batch as well
    rows = make_rows(n, "lmc", ld=4)
    rows[at, 0] = rows[min(at + 5, n - 1), 1] = np.nan
    rc, _, bad = encode_rows_guarded(mc, gpu_ctx, rows, "lmc", 3, software)
    assert rc == mc._lib.MC_ERR_INVALID and bad == at
    b = gpu_ctx.batch([0, at, n - at])
    cols = [np.ascontiguousarray(rows[:, k], np.float32) for k in range(4)]
    b.upload_columns(*cols)
    rc, _, bad = encode_batch_guarded(mc, gpu_ctx, b, "lmc", 3, software)
    assert rc == mc._lib.MC_ERR_INVALID and bad == at
    # a buffer one byte short: MC_ERR_SPACE with the size needed, nothing written
    rows = make_rows(9, "lmc", ld=4)
    d_rows = gpu_ctx.device_buffer(rows.nbytes)
    d_rows.from_host(rows)
    out = guarded(gpu_ctx, 227 + 9 * 34)
    s, o = LAS.xyz3(None, 0.01), LAS.xyz3(None, 0.0)
    P = mc._lib.ptr
    rc = gpu_ctx.lib.mc_las_encode(gpu_ctx.handle, d_rows.ptr, 4, 9, 3, P(s, c_double), P(o, c_double), 65535.0, 0.0,
                                   software, *DATE, inner(out), 227 + 9 * 34 - 1, None)
    assert rc == mc._lib.MC_ERR_SPACE and str(227 + 9 * 34).encode() in gpu_ctx.lib.mc_last_error()
    assert (open_guard(out, 227 + 9 * 34) == 0xA5).all()
    d_rows.close()


# ---- 6. decode ---------------------------------------------------------------------------------------------
def decode_guarded(mc, ctx, data):
    h = mc.las._probe(data)
    d_file = mc.ingest._upload_file(ctx, data)
    rows = guarded(ctx, h.n_points * 40)
    P = mc._lib.ptr
    rc = ctx.lib.mc_las_decode(ctx.handle, d_file.ptr, len(data), h.point_format, h.record_length, h.offset_to_points,
                               h.n_points, P(h.scale, c_double), P(h.offset, c_double), inner(rows), 5)
    d_file.close()
    got = open_guard(rows, h.n_points * 40).view(np.float64).reshape(h.n_points, 5)
    assert rc == 0, ctx.lib.mc_last_error()
    return got


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_decode_every_alignment(mc, gpu_ctx, fmt):
    for n in [0, 1, 7, 8, 9, TD - 1, TD, TD + 1, 2 * TD + 3]:
        rows = make_rows(n, "csim", seed=fmt)
        for extra in (0, 2):
            for at in range(227, 243):
                data = LAS.encode(rows, "csim", 0.001, [500000.0, -3.25, 0.0], fmt, reclen=LAS.NOMINAL[fmt] + extra,
                                  offset_to_points=at)
                want = LAS.decode(data)[1]
                got = decode_guarded(mc, gpu_ctx, data)
                assert np.array_equal(LAS.bits(got), LAS.bits(want)), (n, extra, at)
    # a record length far above the nominal one: the tile does not fit LDS, the records are read in place
    rows = make_rows(300, "csim", seed=9)
    data = LAS.encode(rows, "csim", fmt=fmt, reclen=100, offset_to_points=230)
    assert np.array_equal(LAS.bits(decode_guarded(mc, gpu_ctx, data)), LAS.bits(LAS.decode(data)[1]))
    got = mc.read_las(data, context=gpu_ctx)
    assert (got.point_format, got.record_length, got.offset_to_points, got.n_points) == (fmt, 100, 230, 300)
    assert got.system_identifier == "OTHER" and got.generating_software.startswith("mcdeskew") and got.version == (1, 2)
    assert np.array_equal(LAS.bits(got.rows), LAS.bits(LAS.decode(data)[1]))
    h = LAS.parse_header(data)
    assert np.array_equal(got.maxs, h["bounds"][0::2]) and np.array_equal(got.mins, h["bounds"][1::2])


def test_decode_is_not_fused(mc, gpu_ctx):
    """X * scale + offset as one fused multiply-add changes over a quarter of these rows."""
    rng = np.random.default_rng(1)
    X = rng.integers(-2 ** 31, 2 ** 31, 20000)
    assert LAS.fused_differs(X, 0.001, 500000.0) >= 1000
    rec = np.zeros(len(X), LAS.RECORD[3])
    rec["X"], rec["Y"], rec["Z"] = X, X[::-1], np.roll(X, 7)
    rec["gps_time"] = rng.integers(0, 2 ** 37, len(X)) * 1e-9
    s, o = np.full(3, 0.001), np.full(3, 500000.0)
    data = LAS.header(rec, 3, s, o, b"test", *DATE).tobytes() + rec.tobytes()
    got = decode_guarded(mc, gpu_ctx, data)
    want = LAS.decode(data)[1]
    assert np.array_equal(LAS.bits(want[:, 0]), LAS.bits(LAS.unscale(X, 0.001, 500000.0)))
    assert np.array_equal(LAS.bits(got), LAS.bits(want))


def test_decode_to_batch(mc, gpu_ctx, software):
    counts = np.array([0, 300, 0, TD, 2 * TD + 3, 0])
    n = int(counts.sum())
    rows = make_rows(n, "csim", seed=3)
    off = np.concatenate([[0], np.cumsum(counts)])
    for f in range(len(counts)):   # timestamps inside each frame's int32 window, not sorted
        rows[off[f]:off[f + 1], 4] = 10_000_000_000 * (f + 1) + np.random.default_rng(f).integers(0, 2 ** 30, counts[f])
    ts = rows[:, 4].astype(np.int64)
    assert (np.rint((ts * 1e-9) * 1e9) == ts).all()   # exact below 2^37 ns
    data = mc.encode_las(rows, "csim", creation_date=DATE, context=gpu_ctx)
    assert data == LAS.encode(rows, "csim", software=software, year=DATE[0], day=DATE[1])
    want = LAS.decode(data)[1]
    batch, meta = mc.read_las_batch(data, counts=counts, context=gpu_ctx)
    assert meta.rows is None and meta.n_points == n
    cols = np.stack(batch.download_columns(), 1)
    assert np.array_equal(cols.view(np.uint32), want[:, :4].astype(np.float32).view(np.uint32))
    starts = np.array([ts[off[f]] if counts[f] else 0 for f in range(len(counts))])
    assert np.array_equal(batch.frame_starts, starts)
    assert np.array_equal(batch.download_time(), ts - np.repeat(starts, counts))
    # the caller's frame starts, an intensity scale, formats without time
    mine = starts - 7
    batch, _ = mc.read_las_batch(data, counts=counts, frame_start_ns=mine, intensity_scale=1 / 65535, context=gpu_ctx)
    assert np.array_equal(batch.download_time(), ts - np.repeat(mine, counts)) and np.array_equal(batch.frame_starts, mine)
    assert np.array_equal(batch.download_columns()[3].view(np.uint32),
                          (want[:, 3] * (1 / 65535)).astype(np.float32).view(np.uint32))
    batch, _ = mc.read_las_batch(LAS.encode(rows, "csim", fmt=2, reclen=28, offset_to_points=233), counts=counts,
                                 context=gpu_ctx)
    assert not batch.download_time().any() and not batch.frame_starts.any()
    # a span over int32 inside a frame: refused, naming the point
    rows[off[4] + 5, 4] = rows[off[4], 4] + 2 ** 31
    wide = LAS.encode(rows, "csim")
    with pytest.raises(ValueError, match=rf"point {off[4] + 5} \(the first of 1\).*int32"):
        mc.read_las_batch(wide, counts=counts, context=gpu_ctx)
    mc.read_las_batch(wide, counts=counts, frame_start_ns=starts + np.array([0, 0, 0, 0, 2 ** 30, 0]), context=gpu_ctx)
    with pytest.raises(ValueError, match="add up"):
        mc.read_las_batch(data, counts=[n - 1], context=gpu_ctx)
    with pytest.raises(ValueError, match="signature"):
        mc.read_las(b"LASX" + data[4:], context=gpu_ctx)


# ---- 7. round trip and hooks -------------------------------------------------------------------------------
def test_round_trip_into_a_deskew(mc, gpu_ctx, tmp_path):
    p = golden("csim_pathb.npz")
    counts = [0, 700, T + 1, 0, 3]
    b, rows = make_batch(gpu_ctx, counts, "csim", seed=5)
    gpu_ctx.set_imu(p["mid/imu_ts"] - p["mid/imu_ts"][0] + 1_000_000_000 - 50_000_000, p["mid/imu_gyro"])
    path = tmp_path / "cloud.las"
    assert mc.write_las(path, b, variant="csim", scale=1e-6) == 227 + sum(counts) * 34   # float32 metres to the micrometre
    back, meta = mc.read_las_batch(path, counts=counts, frame_start_ns=b.frame_starts, context=gpu_ctx)
    assert np.array_equal(back.download_time(), b.download_time())
    out = gpu_ctx.deskew(back, mode="imu")
    ref = gpu_ctx.deskew(b, mode="imu")
    assert np.array_equal(out.download_time(), ref.download_time())
    got, want = np.stack(out.download_columns()), np.stack(ref.download_columns())
    assert np.array_equal(got[3], np.trunc(want[3]))   # the intensity went through a u16
    # inputs moved by at most half the 1e-6 grid per axis (sqrt(3) / 2 of it through a rotation), outputs
    # below 2000 sqrt(3) < 4096 rounded to float32 (an ulp of at most 2^-12)
    assert np.abs(got[:3].astype(np.float64) - want[:3]).max() <= 1e-6 + 2.0 ** -12
    assert not np.array_equal(want[:3], np.stack(b.download_columns())[:3])                  # the deskew moved the points


def test_save_results_hook(mc, gpu_ctx, software, tmp_path):
    name = "highway_simple"
    with open(os.path.join(GOLDEN, "lmc_run_files.json")) as f:
        ref = json.load(f)[name]
    e = golden(f"lmc_env_{name}.npz")
    tr = traj_of(name)
    sim = mc.LiDARMotionSimulator(dict(CFGS[name]), context=gpu_ctx)
    restore_rng(e)
    res = sim.simulate_frames(e["environment"], tr, sim.lidar_times())
    # this scene has empty frames: LMC:887 skips the merge, so no .las, and everything else as the golden run
    out = tmp_path / "out"
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        sim.save_results(res, str(out), las="device")
    assert digests(str(out)) == {k: v for k, v in ref["files"].items()}
    assert log_lines(log.getvalue().replace(str(out), "<out>")) == log_lines(ref["log"])
    # the aligned rows simulate_frames left on the device, encoded where they are
    al = np.vstack(res["aligned_pointclouds"])
    rows = sim._rows_of(res)
    data = mc.las.encode_las_device_rows(rows.d_aligned, len(al), creation_date=DATE)
    assert data == LAS.encode(np.column_stack([al, np.zeros(len(al))]), "lmc", software=software, year=DATE[0], day=DATE[1])
    # the frames that hold points: the merge happens, merged_aligned.las is the lmc variant of the merged cloud
    keep = [i for i, a in enumerate(res["aligned_pointclouds"]) if len(a)][:6]
    part = {"raw_scans": [res["raw_scans"][i] for i in keep], "aligned_pointclouds": [res["aligned_pointclouds"][i] for i in keep],
            "motion_data": [res["motion_data"][i] for i in keep], "trajectory": tr, "environment": e["environment"]}
    for las, sub in (("device", "dev"), ("laspy", "ref")):
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            sim.save_results(part, str(tmp_path / sub), las=las)
        assert ("LAS format saved successfully" in log.getvalue()) == (las == "device")
    dev, host = digests(str(tmp_path / "dev")), digests(str(tmp_path / "ref"))
    assert sorted(set(dev) - set(host)) == ["merged_aligned.las"] and all(dev[k] == host[k] for k in host)
    data = (tmp_path / "dev" / "merged_aligned.las").read_bytes()
    merged = np.vstack(part["aligned_pointclouds"])
    h = LAS.parse_header(data)
    assert data == LAS.encode(np.column_stack([merged, np.zeros(len(merged))]), "lmc", software=software,
                              year=int(h["year"]), day=int(h["day"]))
    assert int(h["year"]) >= 2024 and (h["scale"] == 0.01).all() and int(h["count"]) == len(merged)


def test_data_exporter_hook(mc, gpu_ctx, software, tmp_path):
    g = golden("csim_export.npz")
    frames = f_frames(mc, g)
    exporter = mc.csim_export.DataExporter({"las_writer": "device"}, context=gpu_ctx)
    exporter.export_point_clouds(frames, str(tmp_path / "cloud"))
    assert sorted(os.listdir(tmp_path)) == ["cloud.csv", "cloud.las", "cloud.pcd", "cloud.xyz"]
    for ext, key in (("pcd", "F_pcd"), ("xyz", "F_xyz_file"), ("csv", "F_csv")):
        assert (tmp_path / f"cloud.{ext}").read_bytes() == g[key].tobytes(), ext
    data = (tmp_path / "cloud.las").read_bytes()
    h = LAS.parse_header(data)
    assert data == LAS.encode(f_rows(g), "csim", software=software, year=int(h["year"]), day=int(h["day"]))
    assert (h["scale"] == 0.001).all()
    empty = tmp_path / "empty"
    empty.mkdir()
    exporter.export_point_clouds([{"timestamp": 0, "points": []}], str(empty / "cloud"))
    assert os.listdir(empty) == []
