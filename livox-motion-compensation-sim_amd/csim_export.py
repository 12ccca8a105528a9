"""The CSIM exports on the device, byte-exact: LivoxLVXWriter.write_lvx_file (lvx / lvx2 / lvx3,
CSIM:235-374) and DataExporter's PCD / XYZ / CSV (CSIM:1603-1715).  CSIM =
livox_mid70_complete_simulator.py.

The reference's writers loop over points in Python (a ``struct.pack`` triple per 14-byte record, an
f-string per PCD line, ``np.savetxt``, ``DataFrame.to_csv``).  Here the records and the text lines
come from gfx950 kernels (csrc/csim_codecs.hpp; include/mcdeskew.h ``mc_csim_lvx_encode`` /
``mc_csim_text_encode``); the host adds the constant headers and writes the bytes.

  LivoxLVXWriter(format_version).write_lvx_file(filename, frames_data, device_info)   CSIM:235-374
  DataExporter(config).export_point_clouds(frames_data, output_prefix)                CSIM:1612-1641
      ._export_pcd / ._export_xyz / ._export_csv(points, filename)                    CSIM:1643-1715
  encode_lvx / encode_text                 the bytes from (N, 5) float64 rows, without a file
  encode_lvx_batch / encode_text_batch     straight from a device Batch (with time and frame starts)
  batch_rows(batch)                        the rows a batch's points stand for
  frames_to_rows(frames_data)              the reference's frame dicts as rows, counts, timestamps, tags

Deviations from the reference: where its write raises halfway (``struct.error`` /
``OverflowError``, leaving a partial file), ``ValueError`` is raised here before the file is opened;
no ``.las`` is written by default (the reference's LASPY_AVAILABLE = False branch; the config key
``'las_writer': 'device'`` adds it through las.write_las, without laspy); ``export_sensor_data`` is
not part of this module.
"""
from __future__ import annotations

from ctypes import c_float, c_int64, c_uint8, c_uint64
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from . import _lib
from ._lib import check, ptr
from .compensator import LiDARPoint  # noqa: F401  (the frames' point type, CSIM:120-129)
from .runtime import Batch, Context, default_context

VERSIONS = {"lvx": 1, "lvx2": 2, "lvx3": 3}     # MC_CSIM_LVX_LEGACY / MC_CSIM_LVX2 / MC_CSIM_LVX3
FORMATS = {"pcd": 0, "xyz": 1, "csv": 2}        # MC_CSIM_PCD / MC_CSIM_XYZ / MC_CSIM_CSV
CSV_HEADER = b"x,y,z,intensity,timestamp\n"     # CSIM:1711
PCD_HEADER = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity timestamp\n"
              "SIZE 4 4 4 4 8\nTYPE F F F F F\nCOUNT 1 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
              "POINTS {n}\nDATA ascii\n")       # CSIM:1648-1659


@dataclass
class DeviceInfo:
    """CSIM:131-143."""
    lidar_sn: str
    device_type: int
    firmware_version: str
    extrinsic_enable: bool
    roll: float
    pitch: float
    yaw: float
    x: float
    y: float
    z: float


def pcd_header(n: int) -> bytes:
    return PCD_HEADER.format(n=int(n)).encode("ascii")


def _version(version: str) -> int:
    if version not in VERSIONS:
        raise ValueError(f"Unsupported format version: {version}")   # CSIM:243
    return VERSIONS[version]


def lvx_layout(counts, version: str = "lvx2") -> np.ndarray:
    """Byte offset of every frame in the file (CSIM:269-374); the last entry is the file size."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    pos = np.zeros(len(counts) + 1, np.int64)
    check(_lib.load().mc_csim_lvx_layout(_version(version), len(counts), ptr(counts, c_int64), ptr(pos, c_int64)),
          "csim_lvx_layout")
    return pos


def _byte(v, what: str) -> int:
    # struct.pack('<B', v) (CSIM:305, 320-321, 373-374) takes an int in 0..255 only
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255:
        raise ValueError(f"{what} must be an int in 0..255, got {v!r}")
    return int(v)


def _device_fields(device_info):
    """lidar_sn as 16 bytes, device_type, extrinsic flag, the six float32 extrinsics (CSIM:302-306,
    332-339)."""
    sn = device_info.lidar_sn.encode("ascii")                 # UnicodeEncodeError is a ValueError
    if len(sn) > 16:
        # (ljust leaves a longer serial number whole and the reference's header grows; not a device layout)
        raise ValueError(f"lidar_sn longer than 16 bytes: {device_info.lidar_sn!r}")
    sn16 = np.frombuffer(sn.ljust(16, b"\x00"), np.uint8).copy()
    ext = np.array([device_info.roll, device_info.pitch, device_info.yaw, device_info.x, device_info.y,
                    device_info.z], np.float64)
    with np.errstate(over="ignore"):
        ext32 = ext.astype(np.float32)
    if (np.isinf(ext32) & ~np.isinf(ext)).any():              # struct.pack('<f') OverflowError
        raise ValueError("an extrinsic parameter overflows float32")
    return sn16, _byte(device_info.device_type, "device_type"), 1 if device_info.extrinsic_enable else 0, ext32


def _timestamps(ts) -> np.ndarray:
    out = []
    for t in ts:
        if isinstance(t, (float, np.floating)) or not 0 <= int(t) < 2 ** 64:   # struct.pack('<Q')
            raise ValueError(f"frame timestamp {t!r} does not fit the u64 field")
        out.append(int(t))
    return np.array(out, np.uint64)


def frames_to_rows(frames_data: List[Dict]):
    """The reference's frame dicts (``points``: List[LiDARPoint], ``timestamp``) as the arrays the
    encoders take: rows (N, 5) float64 = x, y, z, intensity, timestamp (CSIM:1627), counts (F,),
    frame timestamps (F,) uint64 and tags (N,) uint8.  An intensity or tag that is not an int in
    0..255 raises ValueError."""
    counts = np.array([len(fr["points"]) for fr in frames_data], np.int64)
    n = int(counts.sum())
    rows = np.empty((n, 5), np.float64)
    tags = np.empty(n, np.uint8)
    i = 0
    for fr in frames_data:
        for p in fr["points"]:
            rows[i, 0], rows[i, 1], rows[i, 2] = p.x, p.y, p.z
            rows[i, 3] = _byte(p.intensity, "LiDARPoint.intensity")
            rows[i, 4] = p.timestamp
            tags[i] = _byte(p.tag, "LiDARPoint.tag")
            i += 1
    return rows, counts, _timestamps([fr["timestamp"] for fr in frames_data]), tags


def _rows(rows) -> np.ndarray:
    a = np.ascontiguousarray(rows, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 5:
        raise IndexError(f"rows must be (N, >= 5) float64 = x, y, z, intensity, timestamp; got shape {a.shape}")
    return a


def _upload(ctx: Context, a: np.ndarray):
    buf = ctx.device_buffer(max(a.nbytes, 8))
    if a.size:
        buf.from_host(a)
    return buf


def _lvx_call(ctx: Context, size: int, call) -> bytes:
    out = ctx.device_buffer(max(size, 8))
    try:
        check(call(out.ptr, size), "csim_lvx_encode")
        return out.to_host(np.uint8, count=size).tobytes()
    finally:
        out.close()


def encode_lvx(rows, counts, timestamps_ns, tags, device_info, version: str = "lvx2",
               context: Context | None = None) -> bytes:
    """The file write_lvx_file (CSIM:245-374) writes for frames whose points are ``rows`` (N, >= 5)
    float64, ``counts[f]`` of them per frame, stamped ``timestamps_ns[f]``; ``tags`` (N,) uint8 or
    None = 0.  Raises ValueError where the reference's write raises."""
    ver = _version(version)
    a = _rows(rows)
    counts = np.ascontiguousarray(counts, np.int64)
    ts = _timestamps(timestamps_ns)
    if counts.ndim != 1 or (counts < 0).any() or int(counts.sum()) != len(a) or len(ts) != len(counts):
        raise ValueError("counts must be non-negative, add up to the rows, and come with one timestamp per frame")
    sn, dtype, ext_on, ext = _device_fields(device_info)
    t = None if tags is None else np.ascontiguousarray(tags, np.uint8)
    if t is not None and t.shape != (len(a),):
        raise ValueError(f"one tag per row expected, got shape {t.shape}")
    ctx = context or default_context()
    size = int(lvx_layout(counts, version)[-1])
    d_rows = _upload(ctx, a)
    d_tags = None
    try:
        if t is not None:
            d_tags = _upload(ctx, t)
        return _lvx_call(ctx, size, lambda o, nb: ctx.lib.mc_csim_lvx_encode(
            ctx.handle, ver, d_rows.ptr, a.shape[1], len(counts), ptr(counts, c_int64), ptr(ts, c_uint64),
            d_tags.ptr if d_tags is not None else None, ptr(sn, c_uint8), dtype, ext_on, ptr(ext, c_float), o, nb))
    finally:
        d_rows.close()
        if d_tags is not None:
            d_tags.close()


def encode_lvx_batch(batch: Batch, device_info, version: str = "lvx2", tags=None) -> bytes:
    """The same file from a device batch's float32 columns (mc_csim_lvx_encode_batch): the bytes of
    :func:`encode_lvx` applied to :func:`batch_rows`, each frame stamped with its frame start
    (frame['timestamp'], CSIM:2049); ``tags`` (N,) uint8 in dense point order, or None = 0."""
    ctx = batch.ctx
    ver = _version(version)
    ts = _timestamps(_frame_starts(batch))
    sn, dtype, ext_on, ext = _device_fields(device_info)
    size = int(lvx_layout(batch.counts, version)[-1])
    d_tags = None
    try:
        if tags is not None:
            t = np.ascontiguousarray(tags, np.uint8)
            if t.shape != (batch.n_points,):
                raise ValueError(f"one tag per point expected, got shape {t.shape}")
            d_tags = _upload(ctx, t)
        return _lvx_call(ctx, size, lambda o, nb: ctx.lib.mc_csim_lvx_encode_batch(
            ctx.handle, ver, batch.handle, ptr(ts, c_uint64), d_tags.ptr if d_tags is not None else None,
            ptr(sn, c_uint8), dtype, ext_on, ptr(ext, c_float), o, nb))
    finally:
        if d_tags is not None:
            d_tags.close()


def _text_call(ctx: Context, n_points: int, n_frames: int, fmt: str, call) -> List[bytes]:
    """Per frame its lines.  The first buffer is sized for LiDAR-scale lines; a longer text is
    reported by MC_ERR_SPACE and written in a second pass of exactly that size."""
    pos = np.zeros(n_frames + 1, np.int64)
    cap = max(n_points * (40 if fmt == "xyz" else 88), 64)
    for _ in range(2):
        out = ctx.device_buffer(cap)
        try:
            rc = call(out.ptr, cap, ptr(pos, c_int64))
            if rc == _lib.MC_ERR_SPACE:
                cap = int(pos[-1])
                continue
            check(rc, "csim_text_encode")
            text = out.to_host(np.uint8, count=int(pos[-1])).tobytes() if pos[-1] else b""
        finally:
            out.close()
        return [text[pos[f]:pos[f + 1]] for f in range(n_frames)]
    raise _lib.McError("csim_text_encode: output size changed between passes")


def _format(fmt: str) -> int:
    if fmt not in FORMATS:
        raise ValueError(f"Unsupported text format: {fmt} (pcd, xyz, csv)")
    return FORMATS[fmt]


def encode_text(rows, fmt: str, counts=None, context: Context | None = None):
    """The point lines of _export_pcd / _export_xyz / _export_csv (CSIM:1643-1715) for ``rows``
    (N, >= 5) float64, without the PCD header or the CSV header line.  ``counts`` None: one cloud,
    returns bytes; else a list with each cloud's lines."""
    code = _format(fmt)
    a = _rows(rows)
    c = np.array([len(a)], np.int64) if counts is None else np.ascontiguousarray(counts, np.int64)
    if c.ndim != 1 or (c < 0).any() or int(c.sum()) != len(a):
        raise ValueError("counts must be non-negative and add up to the rows")
    ctx = context or default_context()
    d_rows = _upload(ctx, a)
    try:
        parts = _text_call(ctx, len(a), len(c), fmt, lambda o, nb, pos: ctx.lib.mc_csim_text_encode(
            ctx.handle, code, d_rows.ptr, a.shape[1], len(c), ptr(c, c_int64), o, nb, pos))
    finally:
        d_rows.close()
    return parts[0] if counts is None else parts


def encode_text_batch(batch: Batch, fmt: str) -> List[bytes]:
    """Each frame's lines from a device batch's float32 columns (mc_csim_text_encode_batch): the bytes
    of :func:`encode_text` applied to :func:`batch_rows`."""
    ctx = batch.ctx
    code = _format(fmt)
    return _text_call(ctx, batch.n_points, batch.n_frames, fmt, lambda o, nb, pos: ctx.lib.mc_csim_text_encode_batch(
        ctx.handle, code, batch.handle, o, nb, pos))


def _frame_starts(batch: Batch) -> np.ndarray:
    s = getattr(batch, "frame_starts", None)
    if s is None:
        raise ValueError("the batch's frame starts are not set (Batch.set_frame_starts)")
    return s


def batch_rows(batch: Batch) -> np.ndarray:
    """The (N, 5) float64 rows a batch's points stand for in the CSIM encoders: [x, y, z,
    trunc(intensity), frame_start_ns[f] + t_ns], the float32 values widened exactly — the row CSIM:1627
    builds from the LiDARPoint of CSIM:1040-1050 (``int()`` of the intensity, ``timestamp + i * 1000``)."""
    if not batch.with_time:
        raise ValueError("the batch has no time column (with_time=True)")
    starts = np.asarray(_frame_starts(batch), np.int64)
    x, y, z, i = batch.download_columns()
    t = batch.download_time().astype(np.int64)
    rows = np.empty((batch.n_points, 5), np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2] = x, y, z
    rows[:, 3] = np.trunc(i.astype(np.float64))
    rows[:, 4] = (np.repeat(starts, batch.counts) + t).astype(np.float64)
    return rows


class LivoxLVXWriter:
    """Drop-in for livox_mid70_complete_simulator.LivoxLVXWriter (CSIM:235-374); the records are
    packed on the GPU."""

    def __init__(self, format_version: str = "lvx2", context: Context | None = None):
        self.format_version = format_version
        self.supported_versions = ["lvx", "lvx2", "lvx3"]
        if format_version not in self.supported_versions:
            raise ValueError(f"Unsupported format version: {format_version}")
        self._context = context

    def write_lvx_file(self, filename: str, frames_data: List[Dict], device_info):
        rows, counts, ts, tags = frames_to_rows(frames_data)
        data = encode_lvx(rows, counts, ts, tags, device_info, self.format_version, self._context)
        with open(filename, "wb") as f:   # opened only once the bytes exist: no partial file
            f.write(data)


class DataExporter:
    """Drop-in for livox_mid70_complete_simulator.DataExporter's point-cloud exports
    (CSIM:1603-1715); the lines are formatted on the GPU."""

    def __init__(self, config: Dict, context: Context | None = None):
        self.config = config
        self.coordinate_system = config.get("coordinate_system", "sensor")   # CSIM:1608
        self._context = context

    def export_point_clouds(self, frames_data: List[Dict], output_prefix: str = "lidar_data"):
        """CSIM:1612-1641: the merged cloud as .pcd, .xyz and .csv (no .las: laspy is absent, the
        reference's LASPY_AVAILABLE = False); no points, no files.  With the config key
        ``'las_writer': 'device'`` the .las of CSIM:1634-1635 is written too, by las.write_las."""
        n = sum(len(fr["points"]) for fr in frames_data)
        if not n:
            return
        points = np.array([[p.x, p.y, p.z, p.intensity, p.timestamp] for fr in frames_data for p in fr["points"]],
                          dtype=np.float64)   # CSIM:1627
        self._export_pcd(points, f"{output_prefix}.pcd")
        if self.config.get("las_writer") == "device":
            self._export_las(points, f"{output_prefix}.las")
        self._export_xyz(points, f"{output_prefix}.xyz")
        self._export_csv(points, f"{output_prefix}.csv")

    def _write(self, points, fmt: str, head, filename: str):
        pts = np.asarray(points, np.float64)
        body = encode_text(pts, fmt, context=self._context) if len(pts) else b""
        with open(filename, "wb") as f:
            f.write(head(len(pts)) + body)

    def _export_pcd(self, points, filename: str):
        self._write(points, "pcd", pcd_header, filename)                  # CSIM:1643-1669

    def _export_las(self, points, filename: str):
        from . import las                                                  # CSIM:1671-1698
        las.write_las(filename, np.asarray(points, np.float64), variant="csim", context=self._context)

    def _export_xyz(self, points, filename: str):
        self._write(points, "xyz", lambda n: b"", filename)               # CSIM:1700-1706

    def _export_csv(self, points, filename: str):
        self._write(points, "csv", lambda n: CSV_HEADER, filename)        # CSIM:1708-1715
