"""Time the LAS 1.2 codec (las; csrc/las.hpp, f8) in both directions, beside the LVX codec's kernels
from the same run (the comparable misaligned-record kernels: 14-byte LVX records against 34-byte LAS
records behind a 227-byte header).

Workload: 600 frames x 100 000 synthetic points (mc_batch_synth, MC_BATCH_WITH_TIME, frame starts at
10 Hz).

    python tools/bench_las.py [--frames 600] [--points 100000] [--repeat 3] [--json out.json]

Cases (kernel time from HIP events, mc_timing_read_codec; median of --repeat):
  las <- rows            mc_las_encode of (N, 5) float64 device rows, csim variant, format 3: 40 + 34 B/point
  las <- batch           mc_las_encode_batch right after a fresh IMU deskew wrote the batch: 20 + 34 B/point
  las -> rows            mc_las_decode: 34 + 40 B/point
  las -> batch           mc_las_decode_batch with the caller's frame starts: 34 + 20 B/point
  lvx v1.1 <- batch      mc_lvx_encode_batch after the same deskew / cold: 16 B/point + the file
  lvx2 -> rows / batch   mc_lvx_decode / mc_lvx_decode_batch: 14 + 41 / 14 + 20 B/point
GB/s = algorithmic bytes over kernel time, set against 8 TB/s.  Once per direction the wall time of the
module call with its host transfers (encode_las from a batch into host bytes; read_las_batch from host
bytes).  No throughput is asked of the LAS kernels in advance: the LVX figures are the yardstick.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time
from ctypes import c_double, c_float, c_int64, c_uint8, c_uint64

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ex, ing, las, ptr = m.csim_export, m.ingest, m.las, m._lib.ptr
    ctx = m.Context(0)
    lib, h = ctx.lib, ctx.handle
    F = args.frames
    counts = np.full(F, args.points, np.int64)
    n = int(counts.sum())
    sim = m.LiDARMotionSimulator({"duration": max(120.0, F / 10.0), "trajectory_type": "figure_eight", "max_speed": 12.0,
                                  "lidar_fps": 10})
    tr = sim.add_sensor_noise(sim.generate_trajectory())
    times = sim.lidar_times()[:F]
    starts = (times * 1e9).astype(np.int64)
    b = ctx.batch(counts, with_time=True)
    b.synth(seed=0, frame_id_base=1000)
    b.set_frame_times(times)
    b.set_frame_starts(starts)
    ts_imu, gyro = m.trajectory.imu_from_trajectory(tr, 200.0)
    ctx.set_imu(ts_imu, gyro)
    out = ctx.batch(counts, with_time=True)
    out.set_frame_starts(starts)
    back = ctx.batch(counts, with_time=True)
    result = {"frames": F, "points": n, "repeat": args.repeat, "cases": {}}

    def kernel_ms(call, before=None):
        if before:
            before()
        rc = call()   # warm-up: scratch allocation, first launch
        if rc != 0:
            raise RuntimeError(f"the codec returned {rc}: {lib.mc_last_error().decode()}")
        ctx.timing(True)
        ctx.read_timing()
        ms = []
        for _ in range(args.repeat):
            if before:
                before()
            call()
            ms.append(ctx.read_timing()["codec_ms"])
        ctx.timing(False)
        return float(np.median(ms)), ms

    def report(name, call, alg_bytes, before=None, wall_s=None):
        ms, all_ms = kernel_ms(call, before)
        gbs = alg_bytes / (ms * 1e-3) / 1e9
        r = {"us": ms * 1e3, "us_all": [v * 1e3 for v in all_ms], "algorithmic_bytes": alg_bytes, "GBps": gbs,
             "hbm_fraction": gbs * 1e9 / HBM_PEAK}
        if wall_s is not None:
            r["wall_ms_with_host_transfers"] = wall_s * 1e3
        result["cases"][name] = r
        print(f"{name:28s} {ms * 1e3:10.1f} us {gbs:8.1f} GB/s {100 * gbs * 1e9 / HBM_PEAK:6.1f} % of 8 TB/s"
              + (f"   module call with host transfers {wall_s * 1e3:8.1f} ms" if wall_s is not None else ""))

    def deskew():
        ctx.deskew(b, out, mode="imu")

    print(f"{F} frames x {args.points} points = {n} points; median of {args.repeat}")
    scale, offset = np.full(3, 0.001), np.zeros(3)
    sp, op = ptr(scale, c_double), ptr(offset, c_double)
    year, day = las._creation(None)
    size = las.HEADER_BYTES + n * 34
    d_file = ctx.device_buffer((size + 15) // 16 * 16)
    bad = c_int64()
    tail = (3, sp, op, 1.0, 1e-9, b"mcdeskew bench", year, day, d_file.ptr, size, ctypes.byref(bad))

    # ---- LAS ------------------------------------------------------------------------------------------
    t0 = time.perf_counter()
    data = las.encode_las(b, "csim")
    wall_enc = time.perf_counter() - t0
    report("las <- batch (after deskew)", lambda: lib.mc_las_encode_batch(h, out.handle, *tail), n * (20 + 34), deskew,
           wall_enc)
    report("las <- batch (cold)", lambda: lib.mc_las_encode_batch(h, b.handle, *tail), n * (20 + 34))
    d_rows = ctx.device_buffer(n * 40)
    dec = (d_file.ptr, size, 3, 34, las.HEADER_BYTES, n, sp, op)
    report("las -> rows", lambda: lib.mc_las_decode(h, *dec, d_rows.ptr, 5), n * (34 + 40))
    t0 = time.perf_counter()
    las.read_las_batch(data, counts=counts, frame_start_ns=starts, context=ctx)[0].close()
    wall_dec = time.perf_counter() - t0
    del data
    report("las -> batch", lambda: lib.mc_las_decode_batch(h, *dec, 1.0, back.handle, ptr(starts, c_int64), None,
                                                           ctypes.byref(bad)), n * (34 + 20), None, wall_dec)
    # rows for the encoder: x, y, z, intensity, timestamp in ns (the decoded seconds x 1e9 would do as well; the
    # LVX2 decoder below leaves exactly the CSIM rows)
    ts, ids = starts.astype(np.uint64), np.arange(F, dtype=np.uint64)
    sn, dtype, ext_on, ext = ex._device_fields(ex.DeviceInfo("3JEDK7M00100451", 1, "", True, 0.01, -0.02, 1.5, 1.2, -0.3, 1.8))
    lsize = int(ex.lvx_layout(counts, "lvx2")[-1])
    d_lvx = ctx.device_buffer((lsize + 15) // 16 * 16)
    assert lib.mc_csim_lvx_encode_batch(h, ex.VERSIONS["lvx2"], b.handle, ptr(ts, c_uint64), None, ptr(sn, c_uint8), dtype,
                                        ext_on, ptr(ext, c_float), d_lvx.ptr, lsize) == 0, lib.mc_last_error()
    head = d_lvx.to_host(np.uint8, count=lsize).tobytes()
    fmt, pos, slots, _, fts, _ = ing._lvx_index(head)
    del head
    pp, cp, tp = ptr(pos, c_int64), ptr(counts, c_int64), ptr(fts, c_int64)
    d_tags = ctx.device_buffer(n)
    report("lvx2 -> rows", lambda: lib.mc_lvx_decode(h, fmt, d_lvx.ptr, lsize, F, pp, cp, tp, 1000, d_rows.ptr, 5,
                                                     d_tags.ptr), n * (14 + 41))
    report("las <- rows", lambda: lib.mc_las_encode(h, d_rows.ptr, 5, n, *tail), n * (40 + 34))
    report("lvx2 -> batch", lambda: lib.mc_lvx_decode_batch(h, fmt, d_lvx.ptr, lsize, F, pp, cp, tp, 1000, back.handle,
                                                            None), n * (14 + 20))
    for x in (d_lvx, d_tags, d_rows, d_file):
        x.close()
    # ---- LVX v1.1 encode, the writer the README's 0.65-0.71 is about -------------------------------------
    vsize = int(m.codecs.lvx_layout(counts)[-1])
    d_v11 = ctx.device_buffer(vsize)
    enc = lambda src: lib.mc_lvx_encode_batch(h, src.handle, ptr(ids, c_uint64), ptr(ts, c_uint64), d_v11.ptr, vsize)  # noqa: E731
    report("lvx v1.1 <- batch (after deskew)", lambda: enc(out), 16 * n + vsize, deskew)
    report("lvx v1.1 <- batch (cold)", lambda: enc(b), 16 * n + vsize)
    d_v11.close()

    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    for x in (b, out, back):
        x.close()


if __name__ == "__main__":
    main()
