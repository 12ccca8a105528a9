"""LAS 1.2 on the device, without laspy: the files of
LiDARMotionSimulator.save_las (LMC:950-963) and DataExporter._export_las (CSIM:1671-1698) — both thin
laspy calls in the reference — written from device float64 rows or a Batch, and read back into rows
or a Batch (csrc/las.hpp, csrc/las_index.cpp; include/mcdeskew.h ``mc_las_*``).

  encode_las(rows_or_batch, variant)   -> bytes of the whole file (227-byte header, no VLRs, records)
  write_las(path, rows_or_batch, ...)  the same into a file, opened only once the bytes exist
  read_las(path_or_bytes)              -> LasData: the header fields and rows (N, 5) float64 =
                                          x, y, z, intensity, gps_time (s)
  read_las_batch(path_or_bytes)        -> (Batch, LasData without rows), ready for Context.deskew

Values, op for op: X = int32(rint((x - offset) / scale)) — subtract, IEEE divide, round half to even,
what laspy's np.round does; intensity truncated toward zero to a u16; every other record byte 0
(return number included), points-by-return 0; header bounds = min / max of the stored integers *
scale + offset.  ``variant="lmc"``: intensity = column 3 * 65535, gps_time 0.0, scale 0.01
(LMC:961); ``variant="csim"``: intensity = column 3, gps_time = column 4 * 1e-9, scale 0.001
(CSIM:1679-1690).  Reading: x = X * scale + offset as a rounded multiply then a rounded add.

What is not claimed.  laspy is not available where this was written, so no file of its making was
compared: byte equality with laspy's own header choices (the identifier strings, the creation date,
the by-return counts) is neither promised nor tested, and the 0.01 scale default of the LMC variant
is laspy's documented default from memory, unchecked.  ``scale`` and ``offset`` are parameters, so
any other writer can be matched.

Refused, where numpy wraps around silently: a coordinate that is not finite, rint(...) outside int32,
an intensity that is NaN or outside 0..65535 after truncation, 2^32 points or more — ValueError naming
the first offending row, and no file is written.  Out of scope: LAS 1.4, formats >= 4, VLRs on write,
LAZ; classification, RGB, return fields and scan angle are written as zeros and skipped on read.
"""
from __future__ import annotations

import ctypes
import datetime
import os
from ctypes import c_double, c_int32, c_int64
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, ptr
from .ingest import _bytes, _upload_file
from .runtime import Batch, Context, default_context

HEADER_BYTES = 227
RECORD_BYTES = {0: 20, 1: 28, 2: 26, 3: 34}
TILE_RECORDS = 512          # csrc/las.hpp kLasTile: records per encode workgroup
DECODE_TILE_RECORDS = 256   # kLasDecTile
# variant -> (intensity multiplier, time multiplier, default scale, source columns)
VARIANTS = {"lmc": (65535.0, 0.0, 0.01, 4), "csim": (1.0, 1e-9, 0.001, 5)}


@dataclass
class LasData:
    point_format: int
    record_length: int
    offset_to_points: int
    n_points: int
    scale: np.ndarray                # (3,)
    offset: np.ndarray               # (3,)
    mins: np.ndarray                 # (3,) as stored in the header
    maxs: np.ndarray                 # (3,)
    version: tuple = (1, 2)
    system_identifier: str = ""
    generating_software: str = ""
    creation: tuple = (0, 0)         # (year, day of year)
    rows: np.ndarray | None = None   # (N, 5) float64 = x, y, z, intensity, gps_time (s)


def _xyz(v, default: float, what: str) -> np.ndarray:
    a = np.full(3, default, np.float64) if v is None else np.broadcast_to(np.asarray(v, np.float64), (3,)).copy()
    if not np.isfinite(a).all() or (what == "scale" and not (a > 0).all()):
        raise ValueError(f"{what} must be finite{' and > 0' if what == 'scale' else ''}, got {v!r}")
    return a


def _creation(creation_date):
    if creation_date is None:
        creation_date = datetime.date.today()
    if isinstance(creation_date, (datetime.date, datetime.datetime)):
        return creation_date.year, creation_date.timetuple().tm_yday
    year, day = (int(v) for v in creation_date)
    if not (0 <= year <= 65535 and 0 <= day <= 366):
        raise ValueError(f"creation_date (year, day of year) out of range: {creation_date!r}")
    return year, day


def _plan(src, variant, scale, offset, point_format):
    """Everything checked before a context is touched -> (rows or None, n, multipliers, scale, offset)."""
    if variant not in VARIANTS:
        raise ValueError(f"Unknown LAS variant: {variant!r} ('lmc' = save_las, 'csim' = _export_las)")
    imul, tmul, dscale, need = VARIANTS[variant]
    if point_format not in RECORD_BYTES:
        raise ValueError(f"point_format {point_format!r}: formats 0 to 3 are written")
    s, o = _xyz(scale, dscale, "scale"), _xyz(offset, 0.0, "offset")
    if isinstance(src, Batch):
        if tmul != 0.0 and not src.with_time:
            raise ValueError("the csim variant needs a batch with a time column (with_time=True)")
        if tmul != 0.0 and getattr(src, "frame_starts", None) is None:
            raise ValueError("the batch's frame starts are not set (Batch.set_frame_starts)")
        a, n = None, src.n_points
    else:
        a = np.asarray(src)
        if a.ndim != 2 or a.shape[1] < need:
            raise IndexError(f"rows must be (N, >= {need}) = x, y, z, intensity{', timestamp' if need == 5 else ''}; "
                             f"got shape {a.shape}")
        n = a.shape[0]
    if n >= 2 ** 32:
        raise ValueError(f"LAS 1.2 stores the point count as a u32: {n} points do not fit")
    return a, n, imul, tmul, s, o


def encode_las(rows_or_batch, variant: str = "lmc", scale=None, offset=None, point_format: int = 3,
               creation_date=None, context: Context | None = None) -> bytes:
    """The LAS 1.2 file of ``rows_or_batch``: (N, >= 4) float64 rows x, y, z, intensity (``csim``:
    (N, >= 5), column 4 = timestamp in ns) or a device Batch (``csim``: with time and frame starts).
    ``scale`` / ``offset``: a number or three (defaults: the variant's scale, offset 0);
    ``creation_date``: a date or (year, day of year), default today.  Raises ValueError naming the
    first row LAS cannot hold (module docstring)."""
    a, n, imul, tmul, s, o = _plan(rows_or_batch, variant, scale, offset, point_format)
    if a is None:
        return _encode(rows_or_batch.ctx, rows_or_batch, None, 0, n, imul, tmul, s, o, point_format, creation_date)
    ctx = context or default_context()
    a = np.ascontiguousarray(a, dtype=np.float64)
    d_rows = ctx.device_buffer(max(a.nbytes, 8))
    try:
        if a.size:
            d_rows.from_host(a)
        return _encode(ctx, None, d_rows, a.shape[1], n, imul, tmul, s, o, point_format, creation_date)
    finally:
        d_rows.close()


def encode_las_device_rows(d_rows, n: int, ld: int = 4, variant: str = "lmc", scale=None, offset=None,
                           point_format: int = 3, creation_date=None) -> bytes:
    """:func:`encode_las` of (n, ld) float64 rows already on the device (a DeviceBuffer), e.g. the
    aligned rows simulate_frames left there."""
    _, n, imul, tmul, s, o = _plan(np.broadcast_to(np.zeros((1, 1)), (int(n), int(ld))), variant, scale, offset,
                                   point_format)
    if d_rows.nbytes < n * ld * 8:
        raise ValueError("device buffer smaller than the rows")
    return _encode(d_rows.ctx, None, d_rows, ld, n, imul, tmul, s, o, point_format, creation_date)


def _encode(ctx, batch, d_rows, ld, n, imul, tmul, s, o, point_format, creation_date) -> bytes:
    year, day = _creation(creation_date)
    from . import __version__
    software = f"mcdeskew {__version__}".encode("ascii")[:32]
    size = HEADER_BYTES + n * RECORD_BYTES[point_format]
    bad = c_int64(-1)
    tail = (point_format, ptr(s, c_double), ptr(o, c_double), imul, tmul, software, year, day)
    out = ctx.device_buffer(size)
    try:
        if batch is not None:
            rc = ctx.lib.mc_las_encode_batch(ctx.handle, batch.handle, *tail, out.ptr, size, ctypes.byref(bad))
        else:
            rc = ctx.lib.mc_las_encode(ctx.handle, d_rows.ptr, ld, n, *tail, out.ptr, size, ctypes.byref(bad))
        check(rc, "encode_las")
        return out.to_host(np.uint8, count=size).tobytes()
    finally:
        out.close()


def write_las(path, rows_or_batch, variant: str = "lmc", scale=None, offset=None, point_format: int = 3,
              creation_date=None, context: Context | None = None) -> int:
    """:func:`encode_las` into ``path``; the file is opened only once the bytes exist (a refused cloud
    leaves no file and touches none that is there).  Returns the file size."""
    data = encode_las(rows_or_batch, variant, scale, offset, point_format, creation_date, context)
    with open(os.fspath(path), "wb") as f:
        f.write(data)
    return len(data)


def _probe(data: bytes) -> LasData:
    lib = _lib.load()
    raw = np.frombuffer(data, np.uint8)
    fmt, rl, off, n = c_int32(), c_int32(), c_int64(), c_int64()
    s, o, b = np.zeros(3), np.zeros(3), np.zeros(6)
    p = raw.ctypes.data_as(ctypes.c_void_p) if len(raw) else None
    check(lib.mc_las_probe(p, len(raw), ctypes.byref(fmt), ctypes.byref(rl), ctypes.byref(off), ctypes.byref(n),
                           ptr(s, c_double), ptr(o, c_double), ptr(b, c_double)), "read_las", lib)
    text = lambda at: data[at:at + 32].split(b"\x00")[0].decode("ascii", "replace")   # noqa: E731
    return LasData(fmt.value, rl.value, off.value, n.value, s, o, b[1::2].copy(), b[0::2].copy(),
                   (data[24], data[25]), text(26), text(58),
                   (int.from_bytes(data[92:94], "little"), int.from_bytes(data[90:92], "little")))


def read_las(path_or_bytes, context: Context | None = None) -> LasData:
    """Decode a LAS 1.0 - 1.3 file of point format 0..3 (any offset to point data, any record length
    >= the format's) into ``LasData.rows`` (N, 5) float64.  A malformed header raises ValueError before
    anything is launched."""
    data = _bytes(path_or_bytes)
    h = _probe(data)
    ctx = context or default_context()
    d_file = _upload_file(ctx, data)
    d_rows = None
    try:
        d_rows = ctx.device_buffer(max(h.n_points * 40, 8))
        check(ctx.lib.mc_las_decode(ctx.handle, d_file.ptr, len(data), h.point_format, h.record_length,
                                    h.offset_to_points, h.n_points, ptr(h.scale, c_double), ptr(h.offset, c_double),
                                    d_rows.ptr, 5), "read_las")
        h.rows = d_rows.to_host(np.float64, count=h.n_points * 5).reshape(h.n_points, 5)
    finally:
        d_file.close()
        if d_rows is not None:
            d_rows.close()
    return h


def read_las_batch(path_or_bytes, counts=None, frame_start_ns=None, intensity_scale: float = 1.0,
                   context: Context | None = None):
    """The same file straight into a device Batch with time: x, y, z = float32 of the float64 values,
    intensity = float32(intensity * ``intensity_scale``) (1 / 65535 undoes the LMC variant's scaling),
    t_ns = int64(rint(gps_time * 1e9)) - frame_start_ns[f], which must fit int32 (ValueError naming the
    point).  ``counts``: the frames' sizes (default one frame); ``frame_start_ns`` defaults to each
    frame's first point's time.  Returns (batch, LasData without rows)."""
    data = _bytes(path_or_bytes)
    h = _probe(data)
    c = np.array([h.n_points], np.int64) if counts is None else np.ascontiguousarray(counts, np.int64)
    if c.ndim != 1 or (c < 0).any() or int(c.sum()) != h.n_points:
        raise ValueError(f"counts must be non-negative and add up to the {h.n_points} points of the file")
    starts = None
    if frame_start_ns is not None:
        starts = np.ascontiguousarray(np.atleast_1d(frame_start_ns), np.int64)
        if len(starts) != len(c):
            raise ValueError("one frame start per frame expected")
    ctx = context or default_context()
    d_file = _upload_file(ctx, data)
    try:
        batch = ctx.batch(c, with_time=True)
        used = np.zeros(len(c), np.int64)
        bad = c_int64(-1)
        check(ctx.lib.mc_las_decode_batch(ctx.handle, d_file.ptr, len(data), h.point_format, h.record_length,
                                          h.offset_to_points, h.n_points, ptr(h.scale, c_double),
                                          ptr(h.offset, c_double), float(intensity_scale), batch.handle,
                                          ptr(starts, c_int64), ptr(used, c_int64), ctypes.byref(bad)),
              "read_las_batch")
        batch.frame_starts = used
    finally:
        d_file.close()
    return batch, h
