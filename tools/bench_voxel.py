"""Time the voxel-grid filter (voxel; csrc/voxel.hpp) on BASELINE config 2's globally deskewed batch:
urban_complex figure_eight, 600 frames x 100 000 synthetic points, pose_slerp.

    python tools/bench_voxel.py [--frames 600] [--points 100000] [--repeat 3] [--json out.json]
                                [--libs a/libmcdeskew.so,b/libmcdeskew.so]

For each voxel size h in {0.05, 0.2, 1.0}, once right after a fresh deskew wrote the batch and once cold
(another 1.2 GB deskew output written in between): the event time of every phase (insert with the table
reset, rank, accumulate; mc_timing_read_voxel), their sum, the wall time of the build call (which also
holds its two host synchronisations), M, points/s over the phase sum, and the accumulate phase's atomic
bytes over its time (36 B per point: four 64-bit adds and one 32-bit add).  Then the finalise phase of
both emits.  Median of --repeat.  Last, the NumPy restatement of tests/voxel.py on ONE frame of the same
cloud on this box's CPU, labelled as such.

--libs: an interleaved, order-shuffled A/B of builds of the library (two checkouts, or one voxel.hip
compiled two ways) on the build alone at --size (default 0.2); a path given twice (a.so,a.so) is the A/A
spread.  Outputs are checked identical.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0.05, 0.2, 1.0)
ATOMIC_BYTES_PER_POINT = 4 * 8 + 4
SCENARIO = {"duration": 120.0, "trajectory_type": "figure_eight", "environment_complexity": "complex",
            "max_speed": 12.0, "lidar_fps": 10}


def setup(m, lib_path, frames, points):
    ctx = m.Context(0, lib_path=lib_path)
    counts = np.full(frames, points, np.int64)
    sim = m.LiDARMotionSimulator(dict(SCENARIO, duration=max(120.0, frames / 10.0)), context=ctx)
    tr = sim.add_sensor_noise(sim.generate_trajectory())
    b = ctx.batch(counts, with_time=True)
    b.synth(seed=0, frame_id_base=1000)
    b.set_frame_times(sim.lidar_times()[:frames])
    ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])
    out, other = ctx.batch(counts, with_time=True), ctx.batch(counts, with_time=True)
    return ctx, b, out, other


def timed_build(ctx, out, h, before):
    before()
    ctx.sync()
    ctx.read_timing_voxel()
    ctx.timing(True)
    t0 = time.perf_counter()
    cloud = ctx.voxel_downsample(out, h)
    wall = time.perf_counter() - t0
    ctx.timing(False)
    t = ctx.read_timing_voxel()
    return cloud, t, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--libs", default=None)
    ap.add_argument("--size", type=float, default=0.2, help="the voxel size of the --libs comparison")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    n = args.frames * args.points
    result = {"frames": args.frames, "points": n, "repeat": args.repeat, "cases": {}}

    if args.libs:
        libs = [x for x in args.libs.split(",") if x]
        arms = [(f"{os.path.basename(lib)}#{k}", setup(m, lib, args.frames, args.points)) for k, lib in enumerate(libs)]
        for _, (ctx, b, out, _) in arms:
            ctx.deskew(b, out, mode="pose_slerp")
            ctx.voxel_downsample(out, args.size)   # warm-up: the scratch allocation
        times = {name: [] for name, _ in arms}
        order = list(range(len(arms)))
        rng = random.Random(1)
        for _ in range(args.rounds):
            rng.shuffle(order)
            for k in order:
                name, (ctx, b, out, _) = arms[k]
                _, t, _ = timed_build(ctx, out, args.size, lambda: None)
                times[name].append({p + "_us": t[p + "_ms"] * 1e3 for p in ("insert", "rank", "accumulate")})
        ref = None
        for name, (ctx, b, out, _) in arms:
            cloud = ctx.voxel_downsample(out, args.size)
            got = (cloud.rows(), cloud.point_counts())
            ref = ref or got
            same = np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(got[1], ref[1])
            med = {p: statistics.median(x[p] for x in times[name]) for p in times[name][0]}
            result["cases"][name] = {"median_us": med, "all_us": times[name], "identical_to_first": bool(same)}
            print(f"{name:24s} insert {med['insert_us']:9.1f} us  rank {med['rank_us']:9.1f} us  accumulate "
                  f"{med['accumulate_us']:9.1f} us   {'identical' if same else 'DIFFERS'}", flush=True)
    else:
        ctx, b, out, other = setup(m, None, args.frames, args.points)
        print(f"{args.frames} frames x {args.points} points = {n} points; median of {args.repeat}")
        states = (("after deskew", lambda: ctx.deskew(b, out, mode="pose_slerp")),
                  ("cold", lambda: ctx.deskew(b, other, mode="pose_slerp")))
        ctx.deskew(b, out, mode="pose_slerp")
        for h in SIZES:
            ctx.voxel_downsample(out, h)   # warm-up: the scratch allocation, first launches
            for state, before in states:
                runs = []
                for _ in range(args.repeat):
                    cloud, t, wall = timed_build(ctx, out, h, before)
                    runs.append((t["insert_ms"], t["rank_ms"], t["accumulate_ms"], wall * 1e3))
                ins, rank, acc, wall = (float(np.median([r[k] for r in runs])) for k in range(4))
                total = ins + rank + acc
                r = {"M": cloud.n_voxels, "insert_us": ins * 1e3, "rank_us": rank * 1e3, "accumulate_us": acc * 1e3,
                     "phases_us": total * 1e3, "build_call_wall_us": wall * 1e3, "points_per_s": n / (total * 1e-3),
                     "accumulate_atomic_GBps": n * ATOMIC_BYTES_PER_POINT / (acc * 1e-3) / 1e9,
                     "all_ms": [list(x) for x in runs]}
                result["cases"][f"h={h} {state}"] = r
                print(f"h {h:5.2f} {state:13s} M {cloud.n_voxels:9d}  insert {ins * 1e3:9.1f}  rank {rank * 1e3:9.1f}  "
                      f"accumulate {acc * 1e3:9.1f}  sum {total * 1e3:9.1f} us  call {wall * 1e3:9.1f} us  "
                      f"{r['points_per_s'] / 1e9:6.2f} Gpoint/s  atomics {r['accumulate_atomic_GBps']:7.1f} GB/s", flush=True)
            # the emits of the last build (finalise)
            for name, emit in (("rows", cloud.rows), ("batch", cloud.batch)):
                if name == "rows" and cloud.n_voxels * 32 > (2 << 30):
                    continue   # the host copy of the rows would dominate the run
                ms = []
                for _ in range(args.repeat):
                    ctx.read_timing_voxel()
                    ctx.timing(True)
                    x = emit()
                    ctx.timing(False)
                    ms.append(ctx.read_timing_voxel()["finalise_ms"])
                    del x
                result["cases"][f"h={h} finalise -> {name}"] = {"M": cloud.n_voxels, "us": float(np.median(ms)) * 1e3}
                print(f"h {h:5.2f} finalise -> {name:5s} M {cloud.n_voxels:9d}  {float(np.median(ms)) * 1e3:9.1f} us", flush=True)
        # the NumPy restatement on ONE frame of the same cloud, this box's CPU
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import voxel as V
        rows = out.download_frames(0, 1)
        for h in SIZES:
            t0 = time.perf_counter()
            d = V.downsample(rows, h)
            dt = time.perf_counter() - t0
            result["cases"][f"h={h} numpy restatement, 1 frame"] = {"points": len(rows), "M": len(d["rows"]), "ms": dt * 1e3,
                                                                   "points_per_s": len(rows) / dt}
            print(f"h {h:5.2f} NumPy restatement on ONE frame ({len(rows)} points, this box's CPU): {dt * 1e3:8.1f} ms, "
                  f"{len(rows) / dt / 1e6:6.2f} Mpoint/s, M {len(d['rows'])}", flush=True)

    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
