"""Generate tests/golden/csim_export.npz by running the reference's own writers.

Run in the build container only (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_csim_export.py

The reference is imported at run time, as make_golden.py does; only inputs and the bytes of the files
it writes are stored.  ``LivoxLVXWriter.write_lvx_file`` (CSIM:235-374; lvx, lvx2, lvx3) and
``DataExporter`` (CSIM:1603-1715) run in a temporary directory.

Case F (frames): twelve frames of [0, 1, 0, 2, 255, 256, 257, 767, 768, 769, 3, 0] LiDARPoints —
empty frames first, last and between, the 256-line tile and the 768-record unit +-1.  Coordinates
uniform in +-95 m from a seeded generator with planted values (0.0, -0.0, +-1e-7, -0.9999, values
whose x * 1000 lies within an ulp of an integer from either side, "%.6f" ties), intensities including
0 and 255, tags 0 / 1, point timestamps frame_ts + 1000 i, frame timestamps int(t * 1e9) at 10 Hz.
  F_xyz (N, 3), F_intensity, F_tag, F_timestamp (N,), F_counts, F_frame_ts (12,),
  dev_sn, dev_type, dev_ext_enable, dev_ext (roll, pitch, yaw, x, y, z)
  F_lvx, F_lvx2 (file bytes), F_lvx3_is_lvx2, F_pcd, F_xyz_file, F_csv (export_point_clouds' files)
Case T (text edges): handmade (K, 5) float64 rows passed straight to _export_pcd / _export_xyz /
_export_csv — NaN, +-inf and -0.0 in every column, "%.0f" ties, large values, a denormal, "%.6f" ties
and carries.
  T_rows, T_pcd, T_xyz, T_csv
"""
from __future__ import annotations

import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference  # noqa: E402

COUNTS = [0, 1, 0, 2, 255, 256, 257, 767, 768, 769, 3, 0]


def planted() -> np.ndarray:
    near = []
    for v in (1.005, 0.057, 4.35, 8.7, 12.345, 33.333, 64.001, 81.115, 0.001, 94.999):
        for s in (1.0, -1.0):
            near += [s * v, np.nextafter(s * v, np.inf), np.nextafter(s * v, -np.inf)]
    return np.array([0.0, -0.0, 1e-7, -1e-7, -0.9999, 0.9999, 0.0000005, -0.0000005, 0.0078125, -0.0078125,
                     0.0234375, 0.9999995, 9.9999995, -9.9999995, 0.0009999, -0.0004] + near)


def case_f(csim, tmp):
    rng = np.random.default_rng(20260)
    n = sum(COUNTS)
    xyz = rng.uniform(-95.0, 95.0, (n, 3))
    pl = planted()
    # planted values: down the first rows of the 255-point frame (one per row, cycling the axis) and
    # spread over the 769-point frame
    o4 = sum(COUNTS[:4])
    for k, v in enumerate(pl):
        xyz[o4 + k, k % 3] = v
    o9 = sum(COUNTS[:9])
    for k, v in enumerate(pl):
        xyz[o9 + 5 * k + 1, (k + 1) % 3] = v
    inten = rng.integers(0, 256, n)
    inten[:16] = [0, 255, 0, 255, 1, 254, 128, 7, 0, 255, 100, 9, 10, 99, 200, 255]
    tag = rng.integers(0, 2, n)
    frame_ts = np.array([int((1.7e9 + 0.1 * f) * 1e9) for f in range(len(COUNTS))], np.int64)
    ts = np.concatenate([frame_ts[f] + 1000 * np.arange(c, dtype=np.int64) for f, c in enumerate(COUNTS)])
    dev = csim.DeviceInfo(lidar_sn="3JEDK7M00100451", device_type=1, firmware_version="03.08.0000",
                          extrinsic_enable=True, roll=0.0125, pitch=-0.25, yaw=1.5707963, x=1.2, y=-0.35, z=1.85)
    frames, i = [], 0
    for f, c in enumerate(COUNTS):
        pts = [csim.LiDARPoint(float(xyz[j, 0]), float(xyz[j, 1]), float(xyz[j, 2]), int(inten[j]), int(ts[j]),
                               int(j % 4), int(tag[j])) for j in range(i, i + c)]
        frames.append({"frame_id": f, "timestamp": int(frame_ts[f]), "points": pts})
        i += c
    files = {}
    for ver in ("lvx", "lvx2", "lvx3"):
        p = os.path.join(tmp, f"f.{ver}")
        csim.LivoxLVXWriter(ver).write_lvx_file(p, frames, dev)
        files[ver] = open(p, "rb").read()
    csim.DataExporter({}).export_point_clouds(frames, os.path.join(tmp, "cloud"))
    for ext in ("pcd", "xyz", "csv"):
        files[ext] = open(os.path.join(tmp, f"cloud.{ext}"), "rb").read()
    assert not os.path.exists(os.path.join(tmp, "cloud.las"))
    u8 = lambda b: np.frombuffer(b, np.uint8)  # noqa: E731
    return dict(F_xyz=xyz, F_intensity=inten.astype(np.int64), F_tag=tag.astype(np.int64), F_timestamp=ts,
                F_counts=np.array(COUNTS, np.int64), F_frame_ts=frame_ts, dev_sn=np.array(dev.lidar_sn),
                dev_type=np.int64(dev.device_type), dev_ext_enable=np.bool_(dev.extrinsic_enable),
                dev_ext=np.array([dev.roll, dev.pitch, dev.yaw, dev.x, dev.y, dev.z]),
                F_lvx=u8(files["lvx"]), F_lvx2=u8(files["lvx2"]), F_lvx3_is_lvx2=np.bool_(files["lvx3"] == files["lvx2"]),
                F_pcd=u8(files["pcd"]), F_xyz_file=u8(files["xyz"]), F_csv=u8(files["csv"]))


def rows_t() -> np.ndarray:
    nan, inf = np.nan, np.inf
    base = [1.25, -2.5, 3.75, 100.0, 1.7e18]
    rows = []
    for v in (nan, inf, -inf, -0.0):                       # each in every column
        for c in range(5):
            r = list(base)
            r[c] = v
            rows.append(r)
    rows.append([nan] * 5)
    rows.append([-0.0] * 5)
    rows.append([inf, -inf, nan, -inf, inf])
    ties0 = [0.5, 1.5, 2.5, -0.5, -0.3, 0.3, -1.5, 3.5, 0.49999999999999994, 254.5, 255.5, -2.5]
    for k in range(0, len(ties0), 2):
        rows.append([ties0[k], ties0[k + 1], -ties0[k], ties0[k], ties0[k + 1]])
        rows.append([0.0, 1.0, 2.0, ties0[k + 1], ties0[k]])
    big = [2.0 ** 53 + 2, 1.23e18, 1e22, 1e31, -1e31, 2.0 ** 53 - 1, 9007199254740993.0, 1e15 + 0.5]
    for k, v in enumerate(big):
        r = [float(k), -float(k), 0.5 * k, v, v]
        rows.append(r)
        rows.append([v, -v, v, float(k), float(-k)])
    rows.append([5e-324, -5e-324, 2.2250738585072014e-308, 5e-324, -5e-324])
    rows.append([0.9999995, 9.9999995, 999.9999995, 0.9999995, 9.9999995])
    rows.append([-0.9999995, -9.9999995, -999.9999995, 999.9999995, -0.9999995])
    rows.append([0.0000005, 0.0000015, 0.0000025, 0.0078125, 0.0234375])
    rows.append([99999.9999995, 4293.9999996, 4294.0000004, 4294967.2955, 1e-7])
    rows.append([123456789.125, -98765.4321, 1e9, 1e10 + 0.5, 12345678901234567890.0])
    rows.append([95.0, -95.0, 0.0, 0.0, 0.0])
    rows.append([1.0, 2.0, 3.0, 255.0, 1700000000000001000.0])
    rows.append([1e-3, 1e-4, 1e-5, 1e-6, 1e-7])
    rows.append([-1e-3, -1e-4, -1e-5, -1e-6, -1e-7])
    rows.append([10.0, 100.0, 1000.0, 10000.0, 100000.0])
    rows.append([9.9999994999, 99.9999994999, 999.99999949, 9.5, 10.5])
    return np.array(rows, np.float64)


def case_t(csim, tmp):
    rows = rows_t()
    ex = csim.DataExporter({})
    out = {}
    for ext, fn in (("pcd", ex._export_pcd), ("xyz", ex._export_xyz), ("csv", ex._export_csv)):
        p = os.path.join(tmp, f"t.{ext}")
        fn(rows, p)
        out[ext] = np.frombuffer(open(p, "rb").read(), np.uint8)
    return dict(T_rows=rows, T_pcd=out["pcd"], T_xyz=out["xyz"], T_csv=out["csv"])


def main():
    _, csim = import_reference()
    logging.disable(logging.CRITICAL)
    with tempfile.TemporaryDirectory() as tmp:
        data = case_f(csim, tmp)
        data.update(case_t(csim, tmp))
    path = os.path.join(HERE, "csim_export.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape if hasattr(v, "shape") else v) for k, v in data.items()})


if __name__ == "__main__":
    main()
