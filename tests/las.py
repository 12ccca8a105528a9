"""The LAS 1.2 restatement the LAS tests compare with (numpy structured dtypes written from the ASPRS
LAS 1.2 tables; no laspy): the 227-byte public header block, point formats 0..3, and the value
semantics of the two reference writers (LMC:950-963 save_las, CSIM:1671-1698 _export_las) op for op.

  X = int32(rint((x - offset) / scale))      subtract, IEEE divide, round half to even (np.round)
  intensity = trunc(column 3 * imul) as u16  lmc: imul 65535; csim: imul 1
  gps_time = column 4 * tmul                 lmc: tmul 0 -> 0.0; csim: tmul 1e-9
  x = X * scale + offset                     a rounded multiply, then a rounded add
"""
from fractions import Fraction

import numpy as np

HEADER = np.dtype([("signature", "S4"), ("source_id", "<u2"), ("encoding", "<u2"), ("guid", "V16"),
                   ("major", "u1"), ("minor", "u1"), ("system_id", "S32"), ("software", "S32"),
                   ("day", "<u2"), ("year", "<u2"), ("header_size", "<u2"), ("offset_to_points", "<u4"),
                   ("n_vlr", "<u4"), ("format", "u1"), ("reclen", "<u2"), ("count", "<u4"),
                   ("by_return", "<u4", (5,)), ("scale", "<f8", (3,)), ("offset", "<f8", (3,)),
                   ("bounds", "<f8", (6,))])   # bounds = max x, min x, max y, min y, max z, min z
assert HEADER.itemsize == 227

_BASE = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2"), ("flags", "u1"), ("classification", "u1"),
         ("scan_angle", "i1"), ("user_data", "u1"), ("source_id", "<u2")]
_GPS = [("gps_time", "<f8")]
_RGB = [("R", "<u2"), ("G", "<u2"), ("B", "<u2")]
RECORD = {0: np.dtype(_BASE), 1: np.dtype(_BASE + _GPS), 2: np.dtype(_BASE + _RGB), 3: np.dtype(_BASE + _GPS + _RGB)}
NOMINAL = {f: d.itemsize for f, d in RECORD.items()}
assert NOMINAL == {0: 20, 1: 28, 2: 26, 3: 34}

VARIANTS = {"lmc": (65535.0, 0.0, 0.01), "csim": (1.0, 1e-9, 0.001)}   # imul, tmul, default scale
PAD = 0xEE   # filler of the bytes a reader must skip (between header and records, behind a record)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def fix(v, scale, offset):
    """-> (X int64, refused mask) for one axis."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint((np.asarray(v, np.float64) - offset) / scale)
    ok = (q >= -2147483648.0) & (q <= 2147483647.0)
    return np.where(ok, q, 0.0).astype(np.int64), ~ok


def intensity(col, imul):
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(col, np.float64) * imul
    ok = (t > -1.0) & (t < 65536.0)
    return np.trunc(np.where(ok, t, 0.0)).astype(np.int64), ~ok


def xyz3(v, default):
    return np.full(3, default, np.float64) if v is None else np.broadcast_to(np.asarray(v, np.float64), (3,)).copy()


def records(rows, variant, scale=None, offset=None, fmt=3):
    """rows (N, >= 4 | 5) float64 -> (structured records, refused mask (N,))."""
    imul, tmul, dscale = VARIANTS[variant]
    s, o = xyz3(scale, dscale), xyz3(offset, 0.0)
    rows = np.asarray(rows, np.float64)
    rec = np.zeros(len(rows), RECORD[fmt])
    bad = np.zeros(len(rows), bool)
    for k, name in enumerate("XYZ"):
        X, b = fix(rows[:, k], s[k], o[k])
        rec[name] = X
        bad |= b
    it, b = intensity(rows[:, 3], imul)
    rec["intensity"] = it
    bad |= b
    if fmt & 1:
        rec["gps_time"] = rows[:, 4] * tmul if tmul != 0.0 else 0.0
    return rec, bad


def unscale(X, scale, offset):
    return np.asarray(X).astype(np.float64) * scale + offset   # numpy: two rounded operations


def header(rec, fmt, scale, offset, software, year, day, reclen=None, offset_to_points=227, minor=2):
    h = np.zeros((), HEADER)
    h["signature"], h["major"], h["minor"] = b"LASF", 1, minor
    h["system_id"], h["software"] = b"OTHER", software
    h["day"], h["year"] = day, year
    h["header_size"], h["offset_to_points"] = 227, offset_to_points
    h["format"], h["reclen"], h["count"] = fmt, NOMINAL[fmt] if reclen is None else reclen, len(rec)
    h["scale"], h["offset"] = scale, offset
    if len(rec):
        for k, name in enumerate("XYZ"):
            h["bounds"][2 * k] = unscale(rec[name].max(), scale[k], offset[k])
            h["bounds"][2 * k + 1] = unscale(rec[name].min(), scale[k], offset[k])
    return h


def encode(rows, variant="lmc", scale=None, offset=None, fmt=3, software=b"mcdeskew 0.1.0", year=2024, day=61,
           reclen=None, offset_to_points=227, minor=2):
    """The whole file; ValueError naming the first refused row.  reclen / offset_to_points above the
    nominal values put PAD bytes where a reader must skip."""
    imul, tmul, dscale = VARIANTS[variant]
    s, o = xyz3(scale, dscale), xyz3(offset, 0.0)
    rec, bad = records(rows, variant, s, o, fmt)
    if bad.any():
        raise ValueError(f"row {int(np.flatnonzero(bad)[0])}")
    h = header(rec, fmt, s, o, software, year, day, reclen, offset_to_points, minor)
    body = rec.tobytes()
    if reclen is not None and reclen != NOMINAL[fmt]:
        wide = np.full((len(rec), reclen), PAD, np.uint8)
        wide[:, :NOMINAL[fmt]] = np.frombuffer(body, np.uint8).reshape(len(rec), NOMINAL[fmt])
        body = wide.tobytes()
    return h.tobytes() + bytes([PAD]) * (offset_to_points - 227) + body


def batch_rows(cols, t_ns, counts, frame_start_ns, with_time=True):
    """The rows a batch's points stand for: float32 columns widened, time = float64(start + t_ns)."""
    rows = np.zeros((len(cols[0]), 5), np.float64)
    for k in range(4):
        rows[:, k] = np.asarray(cols[k], np.float32).astype(np.float64)
    if with_time:
        rows[:, 4] = (np.repeat(np.asarray(frame_start_ns, np.int64), counts) + np.asarray(t_ns, np.int64)).astype(np.float64)
    return rows


def parse_header(data):
    return np.frombuffer(data[:227], HEADER)[0]


def decode(data):
    """-> (header, rows (N, 5) float64 = x, y, z, intensity, gps_time)."""
    h = parse_header(data)
    fmt, reclen, at, n = int(h["format"]), int(h["reclen"]), int(h["offset_to_points"]), int(h["count"])
    raw = np.frombuffer(data, np.uint8)[at:at + n * reclen].reshape(n, reclen)[:, :NOMINAL[fmt]]
    rec = np.frombuffer(raw.tobytes(), RECORD[fmt])
    rows = np.zeros((n, 5), np.float64)
    for k, name in enumerate("XYZ"):
        rows[:, k] = unscale(rec[name], h["scale"][k], h["offset"][k])
    rows[:, 3] = rec["intensity"]
    if fmt & 1:
        rows[:, 4] = rec["gps_time"]
    return h, rows


def time_ns(gps):
    """int64(rint(gps_time * 1e9)) -> (values, fits int64)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.rint(np.asarray(gps, np.float64) * 1e9)
    ok = (t >= -9223372036854775808.0) & (t < 9223372036854775808.0)
    return np.where(ok, t, 0.0).astype(np.int64), ok


def fused_differs(X, scale, offset):
    """How many X give another float64 when X * scale + offset is one fused multiply-add (rounded
    once from the exact value) instead of two rounded operations — counted exactly."""
    fs, fo = Fraction(float(scale)), Fraction(float(offset))
    two = unscale(X, scale, offset)
    return sum(1 for x, u in zip(np.asarray(X).tolist(), two.tolist()) if float(Fraction(x) * fs + fo) != u)
