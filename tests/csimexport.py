"""A plain-Python statement of the five CSIM output formats (livox_mid70_complete_simulator.py:
LivoxLVXWriter.write_lvx_file, CSIM:235-374, and DataExporter's PCD / XYZ / CSV, CSIM:1603-1715),
written from the format description with ``struct`` and ``%``.  tests/test_csim_export_cpu.py pins it to
the reference's own files (tests/golden/csim_export.npz); the GPU tests compare the kernels with it on
inputs the golden does not hold.

Rows are (N, >= 5) float64 = x, y, z, intensity, timestamp; frames lie back to back (``counts``).
Where the reference's write raises, these raise ValueError.
"""
import math
import struct

import numpy as np

PCD_HEADER = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity timestamp\n"
              "SIZE 4 4 4 4 8\nTYPE F F F F F\nCOUNT 1 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
              "POINTS {n}\nDATA ascii\n")
CSV_HEADER = "x,y,z,intensity,timestamp\n"


def _sn16(device) -> bytes:
    return device["lidar_sn"].encode("ascii").ljust(16, b"\x00")


def lvx_layout(counts, version="lvx2"):
    """Byte offset of every frame, then the file size."""
    head, per = (60, 12) if version == "lvx" else (88, 45)
    pos = [head]
    for n in counts:
        pos.append(pos[-1] + per + 14 * int(n))
    return np.array(pos, np.int64)


def _intensity(v) -> int:
    t = math.trunc(v) if math.isfinite(v) else -1
    if not 0 <= t <= 255:
        raise ValueError(f"intensity {v!r} does not truncate to 0..255")
    return t


def lvx_bytes(rows, counts, timestamps_ns, tags, device, version="lvx2") -> bytes:
    """``device``: dict with lidar_sn, device_type, extrinsic_enable, roll, pitch, yaw, x, y, z."""
    rows = np.asarray(rows, np.float64)
    tags = np.zeros(len(rows), np.uint8) if tags is None else np.asarray(tags, np.uint8)
    out = []
    if version == "lvx":
        out.append(b"livox_file" + struct.pack("<II", 1, len(counts)) + bytes(10))
        out.append(_sn16(device) + struct.pack("<B", device["device_type"]) + bytes(15))
    elif version in ("lvx2", "lvx3"):
        out.append(b"livox_tech".ljust(10, b"\x00") + b"2.0.0".ljust(6, b"\x00") + struct.pack("<I", 0xAC0EA767) + bytes(4))
        out.append(struct.pack("<II", 50, 1) + _sn16(device)
                   + struct.pack("<BB", device["device_type"], 1 if device["extrinsic_enable"] else 0)
                   + struct.pack("<ffffff", *(device[k] for k in ("roll", "pitch", "yaw", "x", "y", "z"))) + bytes(14))
    else:
        raise ValueError(f"Unsupported format version: {version}")
    i = 0
    for f, (n, ts) in enumerate(zip(counts, timestamps_ns)):
        ts = int(ts)
        if version == "lvx":
            out.append(struct.pack("<QI", ts, int(n)))
        else:
            out.append(struct.pack("<IQI", f, ts, int(n)) + bytes(8))
            out.append(bytes([5, 0, 1, 0]) + struct.pack("<I", 0) + bytes([1, 2]) + bytes(3) + struct.pack("<Q", ts))
        for r in range(i, i + int(n)):
            x, y, z = (float(v) for v in rows[r, :3])
            try:
                if version == "lvx":
                    rec = struct.pack("<fff", x, y, z)
                else:
                    rec = struct.pack("<iii", int(x * 1000), int(y * 1000), int(z * 1000))
            except (struct.error, OverflowError) as e:   # int(nan) raises ValueError itself
                raise ValueError(str(e)) from e
            out.append(rec + bytes([_intensity(float(rows[r, 3])), int(tags[r])]))
        i += int(n)
    return b"".join(out)


def pcd_body(rows) -> bytes:
    return "".join("%.6f %.6f %.6f %.0f %.0f\n" % tuple(float(v) for v in r[:5]) for r in np.asarray(rows)).encode()


def xyz_body(rows) -> bytes:
    return "".join("%.6f %.6f %.6f\n" % tuple(float(v) for v in r[:3]) for r in np.asarray(rows)).encode()


def csv_body(rows) -> bytes:
    return "".join(",".join("" if math.isnan(v) else "%.6f" % v for v in map(float, r[:5])) + "\n"
                   for r in np.asarray(rows)).encode()


BODIES = {"pcd": pcd_body, "xyz": xyz_body, "csv": csv_body}


def text_file(rows, fmt) -> bytes:
    """The whole file of _export_pcd / _export_xyz / _export_csv."""
    head = {"pcd": PCD_HEADER.format(n=len(rows)), "xyz": "", "csv": CSV_HEADER}[fmt]
    return head.encode() + BODIES[fmt](rows)
