"""Ingest on the GPU (ingest.py; csrc/ingest.hpp, f7): LVX files (v1.1, CSIM lvx / lvx2 / lvx3) and ASCII
PCD / XYZ / CSV text decoded on the device, bit for bit against the numpy / float(token) restatement
of tests/ingest.py on the reference-written golden files (tests/golden/codecs.npz, csim_export.npz)
and on synthetic files made by the existing device writers."""
import ctypes
from ctypes import c_int64

import numpy as np
import pytest

import ingest as ING
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 256          # guard bytes on both sides of every output of the edge tests
TILE_LINES = 256     # k_text_parse: lines per workgroup
COUNT_TILE = 16384   # k_text_count / k_text_starts: bytes per workgroup
UNIT = 768           # k_lvx_decode: records per workgroup


@pytest.fixture(scope="module")
def gc():
    return golden("codecs.npz")


@pytest.fixture(scope="module")
def ge():
    return golden("csim_export.npz")


@pytest.fixture(scope="module")
def ing(mc):
    return mc.ingest


def eq_bits(a, b):
    return a.shape == b.shape and np.array_equal(ING.bits(a), ING.bits(b))


# ---- guarded decodes through the C-ABI ---------------------------------------------------------------
def guarded(ctx, nbytes):
    buf = ctx.device_buffer(nbytes + 2 * GUARD)
    buf.from_host(np.full(nbytes + 2 * GUARD, 0xA5, np.uint8))
    return buf


def inner(buf):
    return ctypes.c_void_p(buf.ptr.value + GUARD)


def open_guard(buf, nbytes):
    a = buf.to_host(np.uint8)
    assert (a[:GUARD] == 0xA5).all() and (a[GUARD + nbytes:] == 0xA5).all(), "a decode wrote outside its output"
    buf.close()
    return a[GUARD:GUARD + nbytes].copy()


def lvx_guarded(mc, ctx, data, keep_padding=False, period=0):
    I, P = mc.ingest, mc._lib.ptr
    fmt, pos, slots, ids, ts, dev = I._lvx_index(data)
    d_file = I._upload_file(ctx, data)
    counts = I._lvx_counts(ctx, fmt, d_file, len(data), pos, slots, keep_padding)
    n = int(counts.sum())
    rows, tags = guarded(ctx, n * 40), guarded(ctx, n)
    mc._lib.check(ctx.lib.mc_lvx_decode(ctx.handle, fmt, d_file.ptr, len(data), len(counts), P(pos, c_int64),
                                        P(counts, c_int64), P(ts, c_int64), period, inner(rows), 5, inner(tags)))
    d_file.close()
    return counts, open_guard(rows, n * 40).view(np.float64).reshape(n, 5), open_guard(tags, n)


def text_guarded(mc, ctx, body, sep, cols):
    I = mc.ingest
    d_text = I._upload_file(ctx, body)
    n = I._count_lines(ctx, d_text, len(body))
    rows = guarded(ctx, n * cols * 8)
    bad = c_int64()
    rc = ctx.lib.mc_text_decode(ctx.handle, ord(sep), cols, d_text.ptr, len(body), n, inner(rows), cols, ctypes.byref(bad))
    d_text.close()
    out = open_guard(rows, n * cols * 8).view(np.float64).reshape(n, cols)
    mc._lib.check(rc)
    return out


# ---- 4. LVX v1.1 golden --------------------------------------------------------------------------------
def test_v11_golden(mc, gpu_ctx, gc, ing):
    data = gc["lvx/bytes"].tobytes()
    w, counts, rows, tags = ING.lvx_rows(data)
    assert counts.tolist() == [97, 0, 96, 1, 300, 1000]
    # the restatement itself against the stored inputs: int(clip(p * 1000)) / 1000, reflectivity, timestamps
    i = 0
    for f in range(6):
        p = gc[f"lvx/{f}/points"]
        mm = np.clip(p[:, :3] * 1000, -2147483648.0, 2147483647.0)
        want = np.array([[float(int(v)) / 1000 for v in r] for r in mm]).reshape(len(p), 3)
        assert np.array_equal(ING.bits(rows[i:i + len(p), :3]), ING.bits(want)), f
        refl = np.clip(p[:, 3] * 255, 0, 255).astype(np.int64) if p.shape[1] > 3 else np.full(len(p), 128)
        assert np.array_equal(rows[i:i + len(p), 3], refl / 255.0), f
        assert (rows[i:i + len(p), 4] == float(int(float(gc[f"lvx/{f}/timestamp"]) * 1e9))).all(), f
        i += len(p)
    assert np.array_equal(rows[97 + 96 + 1:97 + 96 + 1 + 300, 3], np.full(300, 128 / 255.0))
    assert np.abs(rows[:, :3]).max() >= 2147483.0   # the clip frame's planted +-3e6 / +-1e300 rows

    got = ing.read_lvx(data, context=gpu_ctx)
    assert got.format == "lvx_v1.1" and got.counts.tolist() == [97, 0, 96, 1, 300, 1000]
    assert got.slots.tolist() == [192, 0, 96, 96, 384, 1056]
    assert eq_bits(got.rows, rows) and np.array_equal(got.tags, tags)
    assert got.timestamps_ns.tolist() == [int(float(gc[f"lvx/{f}/timestamp"]) * 1e9) if f != 1 else -1 for f in range(6)]
    assert got.frame_ids.tolist() == [int(gc[f"lvx/{f}/frame_id"]) for f in range(6)]
    assert got.device_info.lidar_sn == "3GGDJ6K00200101" and got.device_info.device_type == 1

    kept = ing.read_lvx(data, keep_padding=True, context=gpu_ctx)
    wk, ck, rk, tk = ING.lvx_rows(data, keep_padding=True)
    assert kept.counts.tolist() == [192, 0, 96, 96, 384, 1056] == ck.tolist()
    assert eq_bits(kept.rows, rk) and np.array_equal(kept.tags, tk)
    o = np.concatenate([[0], np.cumsum(ck)])
    for f in range(6):   # the extra rows are the zero padding (their timestamp is the package's)
        assert not kept.rows[o[f] + counts[f]:o[f + 1], :4].any(), f

    # a point period: index in frame x period on top of the package timestamp, added in int64
    per = ing.read_lvx(data, point_period_ns=1000, context=gpu_ctx)
    assert eq_bits(per.rows, ING.lvx_rows(data, point_period_ns=1000)[2])

    batch, meta = ing.read_lvx_batch(data, context=gpu_ctx)
    cols = np.stack(batch.download_columns(), 1)
    assert np.array_equal(cols.view(np.uint32), rows[:, :4].astype(np.float32).view(np.uint32))
    assert not batch.download_time().any() and meta.rows is None and np.array_equal(meta.tags, tags)
    assert np.array_equal(batch.frame_starts, got.timestamps_ns)


# ---- 5. CSIM golden, case F ----------------------------------------------------------------------------
@pytest.mark.parametrize("version", ["lvx", "lvx2", "lvx3"])
def test_csim_golden(mc, gpu_ctx, ge, ing, version):
    g = ge
    data = (g["F_lvx"] if version == "lvx" else g["F_lvx2"]).tobytes()
    got = ing.read_lvx(data, context=gpu_ctx)
    assert got.format == ("lvx" if version == "lvx" else "lvx2")   # lvx3 is the same bytes, reported as lvx2
    assert np.array_equal(got.counts, g["F_counts"]) and np.array_equal(got.timestamps_ns, g["F_frame_ts"])
    assert np.array_equal(got.tags, g["F_tag"]) and np.array_equal(got.rows[:, 3], g["F_intensity"])
    if version == "lvx":
        want = g["F_xyz"].astype(np.float32).astype(np.float64)
    else:
        want = np.array([[int(v * 1000) / 1000.0 for v in r] for r in g["F_xyz"]])
        m = np.signbit(g["F_xyz"]) & (g["F_xyz"] == 0)
        assert m.any() and not np.signbit(want[m]).any()   # -0.0 -> +0.0
    assert eq_bits(got.rows[:, :3], want)
    assert eq_bits(got.rows, ING.lvx_rows(data)[2])
    assert np.array_equal(got.rows[:, 4], np.repeat(g["F_frame_ts"], g["F_counts"]).astype(np.float64))
    d = got.device_info
    assert d.lidar_sn == str(g["dev_sn"]) and d.device_type == int(g["dev_type"])
    if version != "lvx":
        assert d.extrinsic_enable == bool(g["dev_ext_enable"])
        assert [d.roll, d.pitch, d.yaw, d.x, d.y, d.z] == [float(np.float32(v)) for v in g["dev_ext"]]
    per = ing.read_lvx(data, point_period_ns=1000, context=gpu_ctx)
    assert np.array_equal(per.rows[:, 4], g["F_timestamp"].astype(np.float64))
    if version == "lvx":   # legacy records round-trip: the re-encoded file is the file
        dev = mc.csim_export.DeviceInfo(d.lidar_sn, d.device_type, "", False, 0, 0, 0, 0, 0, 0)
        again = mc.csim_export.encode_lvx(got.rows, got.counts, got.timestamps_ns, got.tags, dev, "lvx", gpu_ctx)
        assert again == data
    frames = got.frames_data()
    assert [len(fr["points"]) for fr in frames] == g["F_counts"].tolist()
    p = frames[4]["points"][7]
    k = int(g["F_counts"][:4].sum()) + 7
    assert (p.x, p.y, p.z, p.intensity, p.tag, p.ring) == (*got.rows[k, :3], int(g["F_intensity"][k]), int(g["F_tag"][k]), 0)
    batch, meta = ing.read_lvx_batch(data, point_period_ns=1000, context=gpu_ctx)
    cols = np.stack(batch.download_columns(), 1)
    assert np.array_equal(cols.view(np.uint32), got.rows[:, :4].astype(np.float32).view(np.uint32))
    assert np.array_equal(batch.download_time(), np.concatenate([1000 * np.arange(c) for c in g["F_counts"]]))


# ---- 6. text, in-window files ---------------------------------------------------------------------------
def text_cases(gc, ge):
    out = [("F_pcd", ge["F_pcd"].tobytes(), "pcd", 5), ("F_xyz", ge["F_xyz_file"].tobytes(), "xyz", 3),
           ("F_csv", ge["F_csv"].tobytes(), "csv", 5)]
    out += [(k, gc[f"pcd/{k}/bytes"].tobytes(), "pcd", 4) for k in ("random", "f32", "wide", "empty", "specials")]
    return out


def test_text_in_window_files(mc, gpu_ctx, gc, ge, ing):
    for name, data, fmt, cols in text_cases(gc, ge):
        sep = b"," if fmt == "csv" else b" "
        body = ING.body_of(data, fmt)
        lines = ING.text_lines(body)
        assert ING.first_outside(lines, sep) is None, name
        want = ING.parse_lines(lines, sep, cols)
        got = ing.read_points(data, context=gpu_ctx)            # the format from the bytes
        assert got.dtype == np.float64 and eq_bits(got, want), name
        if cols == 4:    # LMC save_pcd lines
            again = mc.codecs.encode_pcd_bodies([got], gpu_ctx)[0] if len(got) else b""
        else:
            rows5 = np.column_stack([got, np.zeros((len(got), 5 - cols))])
            again = mc.csim_export.encode_text(rows5, fmt, context=gpu_ctx) if len(got) else b""
        assert again == body, name
    # F_csv: 19-digit integers with a ".000000" tail — the case the stripped-fraction rule exists for
    first = ING.text_lines(ING.body_of(ge["F_csv"].tobytes(), "csv"))[0].split(b",")[4]
    assert len(first) == 26 and first.endswith(b".000000") and len(first.split(b".")[0]) == 19
    got = ing.read_points(ge["F_csv"].tobytes(), "csv", gpu_ctx)
    assert np.array_equal(got[:, 4], ge["F_timestamp"].astype(np.float64))
    assert (np.signbit(got[:, :3]) & (got[:, :3] == 0)).any()   # "-0.000000" keeps its sign


# ---- 7. text, edge files -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt,cols,total,min_keep", [("T_pcd", "pcd", 5, 63, 50), ("T_xyz", "xyz", 3, 63, 50),
                                                          ("T_csv", "csv", 5, 63, 50), ("tricky", "pcd", 4, 8, 7)])
def test_text_edge_files(gpu_ctx, gc, ge, ing, name, fmt, cols, total, min_keep):
    data = (gc["pcd/tricky/bytes"] if name == "tricky" else ge[name]).tobytes()
    sep = b"," if fmt == "csv" else b" "
    body = ING.body_of(data, fmt)
    head = data[:len(data) - len(body)]
    lines = ING.text_lines(body)
    assert len(lines) == total
    k = ING.first_outside(lines, sep)
    assert k is not None
    with pytest.raises(ValueError, match=rf"line {k} holds a token beyond the device parser"):
        ing.read_points(data, context=gpu_ctx)
    keep = [ln for ln in lines if ING.first_outside([ln], sep) is None]
    assert len(keep) >= min_keep   # a test that filters more is hiding a failure
    rest = b"".join(ln + b"\n" for ln in keep)
    if fmt == "pcd":
        head = head.replace(b"POINTS %d" % total, b"POINTS %d" % len(keep))
    got = ing.read_points(head + rest, context=gpu_ctx)
    assert eq_bits(got, ING.parse_lines(keep, sep, cols))


# ---- 8. shape edges ------------------------------------------------------------------------------------
def seeded_rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = np.empty((n, 5))
    rows[:, :3] = rng.uniform(-120, 120, (n, 3)) * rng.choice([1.0, 1e-3, 37.0], (n, 1))
    rows[:, 3] = rng.integers(0, 256, n)
    rows[:, 4] = 1_700_000_000_000_000_000 + np.arange(n) * 1000
    return rows


def synth_text(mc, ctx, n, fmt, seed=5):
    """Lines made by the existing device writers from a seeded batch's rows."""
    b = ctx.batch([n], with_time=True)
    b.synth(seed=seed, frame_id_base=1000)
    b.set_frame_starts([1_700_000_000_000_000_000])
    return mc.csim_export.encode_text_batch(b, fmt)[0]


@pytest.mark.parametrize("n", [1, TILE_LINES - 1, TILE_LINES, TILE_LINES + 1, 2 * TILE_LINES + 1])
@pytest.mark.parametrize("fmt,cols", [("pcd", 5), ("xyz", 3), ("csv", 5)])
def test_text_line_counts(mc, gpu_ctx, n, fmt, cols):
    body = synth_text(mc, gpu_ctx, n, fmt)
    sep = b"," if fmt == "csv" else b" "
    lines = ING.text_lines(body)
    assert len(lines) == n
    assert eq_bits(text_guarded(mc, gpu_ctx, body, sep.decode(), cols), ING.parse_lines(lines, sep, cols))


def shifted(body, target):
    """body behind one more first line whose leading zeros put a later newline exactly on byte `target`."""
    ends = [i for i, c in enumerate(body) if c == 10]
    base = len(b"1.000000 2.000000 3.000000\n")
    p = max(e for e in ends if e + base <= target)
    return b"0" * (target - p - base) + b"1.000000 2.000000 3.000000\n" + body


def test_text_byte_edges(mc, gpu_ctx):
    body = synth_text(mc, gpu_ctx, 1300, "xyz")
    assert len(body) > 2 * COUNT_TILE

    def check(text, sep=b" ", cols=3):
        lines = ING.text_lines(text)
        got = text_guarded(mc, gpu_ctx, text, sep.decode(), cols)
        assert eq_bits(got, ING.parse_lines(lines, sep, cols))
        return len(lines)

    for target in (COUNT_TILE - 1, COUNT_TILE, 2 * COUNT_TILE - 1, 2 * COUNT_TILE):
        t = shifted(body, target)
        assert t[target] == 10
        assert check(t) == 1301
        assert check(t[:target + 1]) < 1301 and check(t[:target]) < 1301     # the file ends on / just before that newline
    assert check(body[:-1]) == 1300                                            # no trailing newline
    assert check(body.replace(b"\n", b"\r\n")) == 1300                         # \r\n endings
    assert check(body.replace(b"\n", b"\r\n")[:-2]) == 1300 and check(body.replace(b"\n", b"\r\n")[:-1]) == 1300
    lines = body.split(b"\n")[:-1]
    blank = b"\n\r\n\n" + b"\n".join(lines[:200]) + b"\n\n\n\r\n\n" + b"\n".join(lines[200:]) + b"\n\n\r\n\n"
    assert check(blank) == 1300                                                # blank lines: start, middle, end
    assert check(b"\n" * 5000) == 0 and check(b"") == 0 and check(b"\r\n") == 0
    # one ~140-byte line (five 19-digit values) straddling a count-tile edge, between ordinary CSV lines
    csv = synth_text(mc, gpu_ctx, 400, "csv")
    ends = [i for i, c in enumerate(csv) if c == 10]
    cut = max(e for e in ends if e < COUNT_TILE - 20) + 1
    long_line = b",".join(b"%d.%06d" % (1234567890123456789 + 1111 * k, 0) for k in range(5)) + b"\n"
    assert 130 <= len(long_line) <= 140
    t = csv[:cut] + long_line + csv[cut:]
    assert cut < COUNT_TILE < cut + len(long_line)
    assert check(t, b",", 5) == 401
    # tiles of long lines: 256 x 135 bytes do not fit the parse kernel's LDS staging (the direct path)
    assert check(long_line * 300 + csv, b",", 5) == 700


def v11_file(mc, ctx, counts, seed=3):
    rng = np.random.default_rng(seed)
    frames = [{"frame_id": 10 + f, "timestamp": 0.1 * f + 0.05,
               "points": np.column_stack([rng.uniform(1, 50, (c, 3)) * rng.choice([-1, 1], (c, 3)), rng.uniform(0.01, 1, c)])}
              for f, c in enumerate(counts)]
    return mc.codecs.encode_lvx(frames, ctx)


def test_lvx_v11_frame_edges(mc, gpu_ctx):
    counts = [0, 0, 1, 95, 96, 0, 97, 192, 193, 0, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT + 1, 0]
    data = v11_file(mc, gpu_ctx, counts)
    for keep in (False, True):
        for period in (0, 7):
            w, c, rows, tags = ING.lvx_rows(data, keep_padding=keep, point_period_ns=period)
            gcounts, grows, gtags = lvx_guarded(mc, gpu_ctx, data, keep, period)
            assert gcounts.tolist() == c.tolist() == ([-(-n // 96) * 96 for n in counts] if keep else counts)
            assert eq_bits(grows, rows) and np.array_equal(gtags, tags)


@pytest.mark.parametrize("version", ["lvx", "lvx2"])
def test_lvx_csim_frame_edges(mc, gpu_ctx, version):
    counts = np.array([0, 0, 1, UNIT - 1, UNIT, 0, UNIT + 1, 2 * UNIT + 1, 0])
    rows = seeded_rows(int(counts.sum()), 11)
    ts = 1_700_000_000_000_000_000 + 100_000_000 * np.arange(len(counts))
    tags = (np.arange(len(rows)) * 7 % 256).astype(np.uint8)
    dev = mc.csim_export.DeviceInfo("SN123", 3, "", True, 0.5, -0.25, 1.0, 2.0, 3.0, 4.0)
    data = mc.csim_export.encode_lvx(rows, counts, ts, tags, dev, version, gpu_ctx)
    w, c, want, wtags = ING.lvx_rows(data, point_period_ns=1000)
    gcounts, grows, gtags = lvx_guarded(mc, gpu_ctx, data, False, 1000)
    assert gcounts.tolist() == counts.tolist() == c.tolist()
    assert eq_bits(grows, want) and np.array_equal(gtags, wtags) and np.array_equal(gtags, tags)
    assert np.array_equal(grows[:, 3], rows[:, 3])


# ---- 9. the chain ---------------------------------------------------------------------------------------
def shifted_imu(ctx, ge):
    p = golden("csim_pathb.npz")
    ts = p["mid/imu_ts"] - p["mid/imu_ts"][0] + int(ge["F_frame_ts"][0]) - 50_000_000
    ctx.set_imu(ts, p["mid/imu_gyro"])


def uploaded(ctx, counts, rows, starts, t_ns=None):
    b = ctx.batch(counts, with_time=True)
    x, y, z, i = (np.ascontiguousarray(rows[:, k], np.float32) for k in range(4))
    b.upload_columns(x, y, z, i)
    b.upload_time(rows[:, 4].astype(np.int64) - np.repeat(starts, counts) if t_ns is None else t_ns)
    b.set_frame_starts(starts)
    return b


def same_deskew(ctx, a, b):
    oa, ob = ctx.deskew(a, mode="imu"), ctx.deskew(b, mode="imu")
    ca, cb = np.stack(oa.download_columns()), np.stack(ob.download_columns())
    assert np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(oa.download_time(), ob.download_time())
    ia = np.stack(a.download_columns())
    assert not np.array_equal(ca[:3], ia[:3])   # the deskew moved the points


def test_chain_csv_to_deskew(gpu_ctx, ge, ing):
    shifted_imu(gpu_ctx, ge)
    counts = ge["F_counts"]
    data = ge["F_csv"].tobytes()
    rows = ING.parse_lines(ING.text_lines(ING.body_of(data, "csv")), b",", 5)
    off = np.concatenate([[0], np.cumsum(counts)])
    starts = np.array([int(rows[off[f], 4]) if counts[f] else 0 for f in range(len(counts))], np.int64)
    got = ing.read_points_batch(data, counts=counts, context=gpu_ctx)
    assert np.array_equal(got.frame_starts, starts)
    ref = uploaded(gpu_ctx, counts, rows, starts)
    assert np.array_equal(got.download_time(), ref.download_time())
    same_deskew(gpu_ctx, got, ref)
    # the caller's frame starts
    got2 = ing.read_points_batch(data, counts=counts, frame_start_ns=ge["F_frame_ts"], context=gpu_ctx)
    same_deskew(gpu_ctx, got2, uploaded(gpu_ctx, counts, rows, ge["F_frame_ts"]))


def test_chain_lvx2_to_deskew(gpu_ctx, ge, ing):
    shifted_imu(gpu_ctx, ge)
    data = ge["F_lvx2"].tobytes()
    w, counts, rows, tags = ING.lvx_rows(data, point_period_ns=1000)
    got, meta = ing.read_lvx_batch(data, point_period_ns=1000, context=gpu_ctx)
    # t_ns is index x period exactly (the float64 timestamp column of the rows is rounded to 256 ns near 1.7e18)
    t_ns = np.concatenate([1000 * np.arange(c, dtype=np.int64) for c in counts])
    assert np.array_equal(got.download_time(), t_ns)
    same_deskew(gpu_ctx, got, uploaded(gpu_ctx, counts, rows, ge["F_frame_ts"], t_ns))


def test_time_outside_int32_window(gpu_ctx, ge, ing):
    data = ge["F_lvx2"].tobytes()
    with pytest.raises(ValueError, match="int32"):
        ing.read_lvx_batch(data, point_period_ns=2 ** 31 // 700, context=gpu_ctx)   # frame 9 holds 769 points
    # text: the one-frame default start is the first point's time; case F spans 1.1 s, inside the window ...
    ing.read_points_batch(ge["F_csv"].tobytes(), context=gpu_ctx)
    # ... a start 3 s before it is not
    with pytest.raises(ValueError, match=r"line 1: the timestamp minus its frame start does not fit int32"):
        ing.read_points_batch(ge["F_csv"].tobytes(), frame_start_ns=[int(ge["F_frame_ts"][0]) - 3_000_000_000],
                              context=gpu_ctx)


# ---- 10. errors on the device path ------------------------------------------------------------------------
def test_device_path_errors(mc, gpu_ctx, gc, ge, ing):
    xyz = ge["F_xyz_file"].tobytes()
    lines = xyz.split(b"\n")
    lines[299] = lines[299] + b" 4.000000"
    with pytest.raises(ValueError, match="line 300 does not hold 3 fields"):
        ing.read_points(b"\n".join(lines), "xyz", gpu_ctx)
    lines[299] = lines[299].rsplit(b" ", 2)[0]
    with pytest.raises(ValueError, match="line 300 does not hold 3 fields"):
        ing.read_points(b"\n".join(lines), "xyz", gpu_ctx)
    pcd = ge["F_pcd"].tobytes()
    with pytest.raises(ValueError, match="DATA binary"):
        ing.read_points(pcd.replace(b"DATA ascii", b"DATA binary"), context=gpu_ctx)
    with pytest.raises(ValueError, match="POINTS 3078"):
        ing.read_points(pcd[:pcd.rindex(b"\n", 0, len(pcd) - 1) + 1], context=gpu_ctx)
    with pytest.raises(ValueError, match="add up"):
        ing.read_points_batch(pcd, counts=[3000, 77], context=gpu_ctx)
    with pytest.raises(mc.McError, match="MC_BATCH_WITH_TIME"):
        ing.read_points_batch(pcd, with_time=False, context=gpu_ctx)
    with pytest.raises(ValueError, match="CSV header"):
        ing.read_points(b"a,b,c\n1,2,3\n", "csv", gpu_ctx)
    with pytest.raises(ValueError):
        ing.read_lvx(ge["F_lvx2"].tobytes()[:-3], context=gpu_ctx)
    # the context stays usable
    assert len(ing.read_points(xyz, context=gpu_ctx)) == 3078
