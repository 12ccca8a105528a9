"""Ingest: recorded LVX files and ASCII PCD / XYZ / CSV clouds decoded on the
device — the inverse of the writers in codecs.py (LMC:24-272, 932-948) and csim_export.py
(CSIM:235-374, 1603-1715).  file -> device rows or Batch -> deskew -> file, with no per-point work on
the host: the host walks the frame headers (csrc/ingest_index.cpp) and reads the PCD / CSV header
line; the records and the text lines are decoded by gfx950 kernels (csrc/ingest.hpp; include/
mcdeskew.h ``mc_lvx_decode`` / ``mc_text_decode``).

  read_lvx(path_or_bytes)            -> LvxData: format, device_info, frame_ids, timestamps_ns, counts,
                                        rows (N, 5) float64 = x, y, z, intensity, timestamp_ns, tags
  read_lvx_batch(path_or_bytes)      -> (Batch, LvxData without rows), ready for Context.deskew
  read_points(path_or_bytes)         -> (N, C) float64 from a PCD (DATA ascii), CSV or XYZ text
  read_points_batch(path_or_bytes)   -> Batch

What the files do not hold (include/mcdeskew.h): none of the LVX layouts stores a per-point time —
a point's timestamp is its frame's (v1.1: its package's) plus ``point_period_ns`` x (index in frame),
default 0; LVX v1.1 stores no point count and pads a frame's last package with zero records, so the
trailing all-zero records of each frame's last package are dropped — a trailing real point at the
origin with reflectivity 0 goes with them (``keep_padding=True`` keeps every slot).  Decoded mm records
need not re-encode to the same file (both writers truncate x * 1000, and (m / 1000.0) * 1000 can fall
just below m); legacy lvx files and the text formats round-trip.  Text tokens outside the device
parser's window (more than 19 significant or 19 fractional digits, an exponent, other text) raise
ValueError naming the line; there is no host parser to fall back to.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_int32, c_int64, c_uint8, c_uint64
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from . import _lib
from ._lib import check, ptr
from .compensator import LiDARPoint
from .csim_export import DeviceInfo
from .runtime import Batch, Context, default_context

LVX_FORMATS = {0: "lvx_v1.1", 1: "lvx", 2: "lvx2"}   # MC_LVX_V11 / MC_CSIM_LVX_LEGACY / MC_CSIM_LVX2
CSV_HEADER = b"x,y,z,intensity,timestamp"


@dataclass
class LvxData:
    format: str
    device_info: DeviceInfo
    frame_ids: np.ndarray
    timestamps_ns: np.ndarray      # (F,) int64; -1 for a v1.1 frame without a package
    counts: np.ndarray             # (F,) int64
    rows: np.ndarray | None = None  # (N, 5) float64
    tags: np.ndarray | None = None  # (N,) uint8
    slots: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))

    def frames_data(self) -> List[Dict]:
        """The frame dicts LivoxLVXWriter.write_lvx_file takes (CSIM:245): ``ring`` is 0, the formats
        do not store it.  (Builds Python objects per point: for handing a small file on, not a hot path.)"""
        out, i = [], 0
        for f, n in enumerate(self.counts):
            pts = [LiDARPoint(float(r[0]), float(r[1]), float(r[2]), int(r[3]) if self.format != "lvx_v1.1" else float(r[3]),
                              int(r[4]), 0, int(t)) for r, t in zip(self.rows[i:i + n], self.tags[i:i + n])]
            out.append({"frame_id": int(self.frame_ids[f]), "timestamp": int(self.timestamps_ns[f]), "points": pts})
            i += int(n)
        return out


def _bytes(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    if isinstance(src, np.ndarray):
        return src.astype(np.uint8, copy=False).tobytes()
    with open(os.fspath(src), "rb") as f:
        return f.read()


def _upload_file(ctx: Context, data: bytes):
    """The device copy the kernels read: allocated (and zeroed) up to the next multiple of 16 bytes."""
    padded = (len(data) + 15) // 16 * 16
    buf = ctx.device_buffer(max(padded, 16))
    a = np.zeros(max(padded, 16), np.uint8)
    a[:len(data)] = np.frombuffer(data, np.uint8)
    buf.from_host(a)
    return buf


def _lvx_index(data: bytes):
    lib = _lib.load()
    raw = np.frombuffer(data, np.uint8)
    fmt, nf = c_int(), c_int32()
    p = raw.ctypes.data_as(ctypes.c_void_p) if len(raw) else None
    check(lib.mc_lvx_probe(p, len(raw), ctypes.byref(fmt), ctypes.byref(nf)), "read_lvx", lib)
    F = nf.value
    pos, slots = np.zeros(F + 1, np.int64), np.zeros(F, np.int64)
    ids, ts = np.zeros(F, np.uint64), np.zeros(F, np.int64)
    sn, dt, ee, ext = np.zeros(16, np.uint8), c_uint8(), c_uint8(), np.zeros(6, np.float32)
    check(lib.mc_lvx_index(p, len(raw), fmt.value, F, ptr(pos, c_int64), ptr(slots, c_int64), ptr(ids, c_uint64),
                           ptr(ts, c_int64), ptr(sn, c_uint8), ctypes.byref(dt), ctypes.byref(ee), ptr(ext, c_float)),
          "read_lvx", lib)
    dev = DeviceInfo(sn.tobytes().split(b"\x00")[0].decode("ascii", "replace"), dt.value, "", bool(ee.value),
                     *(float(v) for v in ext))
    return fmt.value, pos, slots, ids, ts, dev


def _lvx_counts(ctx, fmt, d_file, nbytes, pos, slots, keep_padding):
    counts = np.zeros(len(slots), np.int64)
    check(ctx.lib.mc_lvx_count(ctx.handle, fmt, d_file.ptr, nbytes, len(slots), ptr(pos, c_int64), ptr(slots, c_int64),
                               1 if keep_padding else 0, ptr(counts, c_int64)), "read_lvx")
    return counts


def read_lvx(path_or_bytes, *, keep_padding: bool = False, point_period_ns: int = 0,
             context: Context | None = None) -> LvxData:
    """Decode an LVX file (v1.1 as LMC:57-272 writes it; CSIM's lvx / lvx2 / lvx3, CSIM:256-374) into
    (N, 5) float64 rows and tags.  A malformed file raises ValueError before anything is launched."""
    data = _bytes(path_or_bytes)
    fmt, pos, slots, ids, ts, dev = _lvx_index(data)
    ctx = context or default_context()
    d_file = _upload_file(ctx, data)
    d_rows = d_tags = None
    try:
        counts = _lvx_counts(ctx, fmt, d_file, len(data), pos, slots, keep_padding)
        n = int(counts.sum())
        d_rows, d_tags = ctx.device_buffer(max(n * 40, 8)), ctx.device_buffer(max(n, 8))
        check(ctx.lib.mc_lvx_decode(ctx.handle, fmt, d_file.ptr, len(data), len(counts), ptr(pos, c_int64),
                                    ptr(counts, c_int64), ptr(ts, c_int64), int(point_period_ns), d_rows.ptr, 5,
                                    d_tags.ptr), "read_lvx")
        rows = d_rows.to_host(np.float64, count=n * 5).reshape(n, 5)
        tags = d_tags.to_host(np.uint8, count=n)
    finally:
        for b in (d_file, d_rows, d_tags):
            if b is not None:
                b.close()
    return LvxData(LVX_FORMATS[fmt], dev, ids, ts, counts, rows, tags, slots)


def read_lvx_batch(path_or_bytes, *, keep_padding: bool = False, point_period_ns: int = 0,
                   context: Context | None = None):
    """The same file straight into a device Batch (with time): columns = float32 of the row values,
    t_ns = index in frame x point_period_ns (must fit int32: ValueError, nothing launched), frame
    starts = the frame timestamps.  Returns (batch, LvxData with tags and without rows), ready for
    Context.deskew(mode="imu" | "pose_slerp" | "frame")."""
    data = _bytes(path_or_bytes)
    fmt, pos, slots, ids, ts, dev = _lvx_index(data)
    ctx = context or default_context()
    d_file = _upload_file(ctx, data)
    d_tags = None
    try:
        counts = _lvx_counts(ctx, fmt, d_file, len(data), pos, slots, keep_padding)
        n = int(counts.sum())
        batch = ctx.batch(counts, with_time=True)
        d_tags = ctx.device_buffer(max(n, 8))
        check(ctx.lib.mc_lvx_decode_batch(ctx.handle, fmt, d_file.ptr, len(data), len(counts), ptr(pos, c_int64),
                                          ptr(counts, c_int64), ptr(ts, c_int64), int(point_period_ns), batch.handle,
                                          d_tags.ptr), "read_lvx_batch")
        batch.frame_starts = ts.copy()
        tags = d_tags.to_host(np.uint8, count=n)
    finally:
        d_file.close()
        if d_tags is not None:
            d_tags.close()
    return batch, LvxData(LVX_FORMATS[fmt], dev, ids, ts, counts, None, tags, slots)


# ---- text ------------------------------------------------------------------------------------------
def _pcd_header(data: bytes):
    """-> (body offset, columns, POINTS) of an ASCII PCD (LMC:932-946, CSIM:1648-1659)."""
    pos, fields, points, kind = 0, None, None, None
    while kind is None:
        end = data.find(b"\n", pos)
        if end < 0:
            raise ValueError("PCD header without a DATA line")
        line = data[pos:end].rstrip(b"\r").decode("ascii", "replace")
        pos = end + 1
        key, _, rest = line.partition(" ")
        if key == "FIELDS":
            fields = rest.split()
        elif key == "POINTS":
            points = int(rest)
        elif key == "DATA":
            kind = rest.strip()
    if kind != "ascii":
        raise ValueError(f"PCD DATA {kind}: only DATA ascii is decoded")
    if fields is None or points is None or not 3 <= len(fields) <= 8:
        raise ValueError("PCD header needs POINTS and 3 to 8 FIELDS")
    return pos, len(fields), points


def _text_layout(data: bytes, fmt):
    """-> (fmt, body offset, separator, columns, expected lines or None)."""
    if fmt is None:
        fmt = "pcd" if data.startswith(b"# .PCD") or data.startswith(b"VERSION") else \
              "csv" if data.startswith(CSV_HEADER) else "xyz"
    if fmt == "pcd":
        off, cols, points = _pcd_header(data)
        return fmt, off, " ", cols, points
    if fmt == "csv":
        end = data.find(b"\n")
        head = data[:end if end >= 0 else len(data)].rstrip(b"\r")
        if head != CSV_HEADER:
            raise ValueError(f"CSV header line {head[:60]!r}: {CSV_HEADER.decode()!r} expected (CSIM:1711)")
        return fmt, (end + 1 if end >= 0 else len(data)), ",", 5, None
    if fmt == "xyz":
        return fmt, 0, " ", 3, None
    raise ValueError(f"Unsupported text format: {fmt} (pcd, xyz, csv)")


def _count_lines(ctx, d_text, nbytes) -> int:
    n = c_int64()
    check(ctx.lib.mc_text_lines(ctx.handle, d_text.ptr, nbytes, ctypes.byref(n)), "read_points")
    return n.value


def read_points(path_or_bytes, fmt: str | None = None, context: Context | None = None) -> np.ndarray:
    """(N, C) float64 of an ASCII cloud: a PCD with DATA ascii (C = its FIELDS: LMC save_pcd 4, CSIM
    _export_pcd 5), a CSV with CSIM's header line (5, an empty field = NaN) or XYZ (3).  ``fmt`` None:
    from the first bytes.  Every value is bit-equal to Python's float(token)."""
    data = _bytes(path_or_bytes)
    fmt, off, sep, cols, expect = _text_layout(data, fmt)
    body = data[off:]
    ctx = context or default_context()
    d_text = _upload_file(ctx, body)
    d_rows = None
    try:
        n = _count_lines(ctx, d_text, len(body))
        if expect is not None and expect != n:
            raise ValueError(f"PCD header says POINTS {expect}, the body holds {n} lines")
        d_rows = ctx.device_buffer(max(n * cols * 8, 8))
        bad = c_int64()
        check(ctx.lib.mc_text_decode(ctx.handle, ord(sep), cols, d_text.ptr, len(body), n, d_rows.ptr, cols,
                                     ctypes.byref(bad)), "read_points")
        return d_rows.to_host(np.float64, count=n * cols).reshape(n, cols)
    finally:
        d_text.close()
        if d_rows is not None:
            d_rows.close()


def read_points_batch(path_or_bytes, fmt: str | None = None, counts=None, frame_start_ns=None,
                      context: Context | None = None, with_time: bool | None = None) -> Batch:
    """The same text into a device Batch: x, y, z, intensity = float32(float64(token)) (XYZ: intensity
    0); a fifth column is the point's timestamp, t_ns = int64(value) - frame_start_ns[f] (default: the
    frame's first point's timestamp), which must fit int32 (ValueError).  ``counts``: the frames'
    sizes (default one frame); they must add up to the line count.  ``with_time`` defaults to
    "the text has a fifth column"; a batch without time handed one raises McError (MC_ERR_STATE)."""
    data = _bytes(path_or_bytes)
    fmt, off, sep, cols, expect = _text_layout(data, fmt)
    body = data[off:]
    ctx = context or default_context()
    d_text = _upload_file(ctx, body)
    try:
        n = _count_lines(ctx, d_text, len(body))
        if expect is not None and expect != n:
            raise ValueError(f"PCD header says POINTS {expect}, the body holds {n} lines")
        c = np.array([n], np.int64) if counts is None else np.ascontiguousarray(counts, np.int64)
        if c.ndim != 1 or (c < 0).any() or int(c.sum()) != n:
            raise ValueError(f"counts must be non-negative and add up to the {n} lines of the text")
        timed = cols >= 5 if with_time is None else bool(with_time)
        batch = ctx.batch(c, with_time=timed)
        starts = None
        if frame_start_ns is not None:
            starts = np.ascontiguousarray(np.atleast_1d(frame_start_ns), np.int64)
            if len(starts) != len(c):
                raise ValueError("one frame start per frame expected")
        used = np.zeros(len(c), np.int64)
        bad = c_int64()
        check(ctx.lib.mc_text_decode_batch(ctx.handle, ord(sep), cols, d_text.ptr, len(body), batch.handle,
                                           ptr(starts, c_int64), ptr(used, c_int64), ctypes.byref(bad)),
              "read_points_batch")
        if timed and cols >= 5:
            batch.frame_starts = used
        return batch
    finally:
        d_text.close()
