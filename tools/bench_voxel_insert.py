"""Time the growth of a voxel cloud (VoxelCloud.insert / .state / .merge; csrc/voxel.hpp "growing a live cloud") on
BASELINE config 2's globally deskewed batch: urban_complex figure_eight, 600 frames x 100 000 synthetic points,
pose_slerp — the batch tools/bench_voxel.py times the one-shot build on.

    python tools/bench_voxel_insert.py [--frames 600] [--points 100000] [--rounds 5] [--sizes 0.05,0.2,1.0]
                                       [--parts 2,6,60] [--json out.json]

For each voxel size h, --rounds interleaved rounds of: the one-shot build (its phases, mc_timing_read_voxel), and the
same points inserted as 2, 6 and 60 equal frame ranges into the cloud of an empty source (the phases of all the
calls together, mc_timing_read_voxel_insert: validate, insert with the table's growth, rank, accumulate; the wall time
with every call's two synchronisations; the growths of the table).  A part is its own batch, synthesised and deskewed
with the frames' own seeds and times, so its points are the whole batch's.  The result is checked against the
one-shot's (M, N, and the counts where they are small enough to bring back).  Medians with the lowest and highest.

Then, on the full one-shot cloud: one further frame of 100 000 points inserted (the frame-to-map case), its phases
beside the one-shot build's time scaled by points; and the records out and in again: the device time of the three
emits that make a state (keys and counts, sums), the device phases of merging those records into the cloud of an empty
source, and the wall time of VoxelCloud.state() and .merge() with their host copies.

The one-shot build against another build of the library is tools/bench_voxel.py --libs.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_voxel import SCENARIO  # noqa: E402

INSERT_PHASES = ("validate", "insert", "rank", "accumulate")
BUILD_PHASES = ("insert", "rank", "accumulate")


def spread(xs):
    return {"median": statistics.median(xs), "low": min(xs), "high": max(xs)}


def fmt(s):
    return f"{s['median']:10.1f} ({s['low']:.1f} .. {s['high']:.1f})"


class Drive:
    """The deskewed batch, whole and as frame ranges."""

    def __init__(self, m, frames, points):
        self.m, self.frames, self.points = m, frames, points
        self.ctx = m.Context(0)
        sim = m.LiDARMotionSimulator(dict(SCENARIO, duration=max(120.0, (frames + 1) / 10.0)), context=self.ctx)
        tr = sim.add_sensor_noise(sim.generate_trajectory())
        self.times = sim.lidar_times()
        self.ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])

    def deskewed(self, f0, f1, time_of=None):
        """Frames [f0, f1) of the drive (seeds and times of their own) as a deskewed batch."""
        counts = np.full(f1 - f0, self.points, np.int64)
        raw = self.ctx.batch(counts, with_time=True)
        raw.synth(seed=0, frame_id_base=1000 + f0)
        raw.set_frame_times(self.times[f0:f1] if time_of is None else self.times[time_of:time_of + f1 - f0])
        out = self.ctx.batch(counts, with_time=True)
        self.ctx.deskew(raw, out, mode="pose_slerp")
        self.ctx.sync()
        return out

    def parts(self, k):
        edges = np.linspace(0, self.frames, k + 1).round().astype(int)
        return [self.deskewed(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def timed(ctx, read, call):
    ctx.sync()
    read()
    ctx.timing(True)
    t0 = time.perf_counter()
    out = call()
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    ctx.timing(False)
    return out, read(), wall


def table(ctx):
    slots, growths = ctypes.c_int64(0), ctypes.c_int64(0)
    ctx.lib.mc_voxel_table(ctx.handle, ctypes.byref(slots), ctypes.byref(growths))
    return slots.value, growths.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="0.05,0.2,1.0")
    ap.add_argument("--parts", default="2,6,60")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    sizes = [float(x) for x in args.sizes.split(",")]
    ks = [int(x) for x in args.parts.split(",")]
    d = Drive(m, args.frames, args.points)
    ctx = d.ctx
    n = args.frames * args.points
    whole = d.deskewed(0, args.frames)
    parts = {k: d.parts(k) for k in ks}
    extra = d.deskewed(args.frames, args.frames + 1, time_of=args.frames - 1)     # a frame the drive has not seen, at its last pose
    result = {"frames": args.frames, "points": n, "rounds": args.rounds, "cases": {}}
    print(f"{args.frames} frames x {args.points} points = {n} points; median (lowest .. highest) of {args.rounds} interleaved rounds; us")

    for h in sizes:
        runs = {"one-shot": []}
        runs.update({f"{k} parts": [] for k in ks})
        ctx.voxel_downsample(whole, h)                                             # warm-up: the scratch allocation
        for _ in range(args.rounds):
            cloud, t, wall = timed(ctx, ctx.read_timing_voxel, lambda: ctx.voxel_downsample(whole, h))
            M = cloud.n_voxels
            counts = cloud.point_counts() if M <= 16_000_000 else None
            runs["one-shot"].append({**{p: t[p + "_ms"] * 1e3 for p in BUILD_PHASES}, "wall": wall * 1e3, "growths": 0})
            for k in ks:
                def grow():
                    c = m.voxel_downsample(np.zeros((0, 4)), h, context=ctx)
                    for part in parts[k]:
                        c.insert(part)
                    return c
                c, t, wall = timed(ctx, ctx.read_timing_voxel_insert, grow)
                ok = c.n_voxels == M and c.n_points == n and (counts is None or np.array_equal(c.point_counts(), counts))
                assert ok, f"h {h}, {k} parts: the grown cloud differs from the one-shot build's"
                runs[f"{k} parts"].append({**{p: t[p + "_ms"] * 1e3 for p in INSERT_PHASES}, "wall": wall * 1e3, "growths": table(ctx)[1]})
        for name, rs in runs.items():
            phases = [p for p in (*INSERT_PHASES, "wall") if p in rs[0]]
            r = {p + "_us": spread([x[p] for x in rs]) for p in phases}
            r["phases_us"] = spread([sum(x[p] for p in phases if p != "wall") for x in rs])
            r["M"], r["growths"] = M, rs[0]["growths"]
            result["cases"][f"h={h} {name}"] = r
            print(f"h {h:5.2f} {name:9s} M {M:9d} growths {r['growths']:2d}  phases {fmt(r['phases_us'])}  wall {fmt(r['wall_us'])}  " +
                  "  ".join(f"{p} {r[p + '_us']['median']:9.1f}" for p in phases if p != "wall"), flush=True)

        # one frame into the full cloud
        one_shot_us = result["cases"][f"h={h} one-shot"]["phases_us"]["median"]
        cloud = ctx.voxel_downsample(whole, h)
        before = table(ctx)
        rs = []
        for _ in range(args.rounds):
            _, t, wall = timed(ctx, ctx.read_timing_voxel_insert, lambda: cloud.insert(extra))
            rs.append({**{p: t[p + "_ms"] * 1e3 for p in INSERT_PHASES}, "wall": wall * 1e3})
        r = {p + "_us": spread([x[p] for x in rs]) for p in (*INSERT_PHASES, "wall")}
        r["phases_us"] = spread([sum(x[p] for p in INSERT_PHASES) for x in rs])
        r["one_shot_scaled_by_points_us"] = one_shot_us * args.points / n
        r["M"], r["table_before"], r["table_after"] = cloud.n_voxels, before, table(ctx)
        result["cases"][f"h={h} one frame into the full cloud"] = r
        print(f"h {h:5.2f} one frame into M {cloud.n_voxels:9d}: phases {fmt(r['phases_us'])}  wall {fmt(r['wall_us'])}  " +
              "  ".join(f"{p} {r[p + '_us']['median']:7.1f}" for p in INSERT_PHASES) +
              f"   the one-shot build scaled by points: {r['one_shot_scaled_by_points_us']:.1f}   table {before} -> {table(ctx)}", flush=True)

        # the records out and in
        cloud = ctx.voxel_downsample(whole, h)
        M = cloud.n_voxels
        bufs = [ctx.device_buffer(M * w) for w in (12, 4, 32)]
        emit, merge, state_wall, merge_wall = [], [], [], []
        for _ in range(args.rounds):
            cloud = ctx.voxel_downsample(whole, h)
            ctx.sync()
            t0 = time.perf_counter()
            m._lib.check(ctx.lib.mc_voxel_emit_f64(ctx.handle, None, bufs[1].ptr, bufs[0].ptr), "emit")
            m._lib.check(ctx.lib.mc_voxel_emit_sums(ctx.handle, bufs[2].ptr), "emit_sums")
            ctx.sync()
            emit.append((time.perf_counter() - t0) * 1e6)
            target = m.voxel_downsample(np.zeros((0, 4)), h, context=ctx)
            new, bad = ctypes.c_int64(0), ctypes.c_int64(0)
            rc, t, _ = timed(ctx, ctx.read_timing_voxel_insert, lambda: ctx.lib.mc_voxel_merge_sums(
                ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, M, ctypes.byref(new), ctypes.byref(bad)))
            m._lib.check(rc, "merge")
            assert new.value == M
            merge.append({p: t[p + "_ms"] * 1e3 for p in INSERT_PHASES})
            del target
        if M <= 16_000_000:                                                        # with the host copies, where they fit a run
            for _ in range(args.rounds):
                cloud = ctx.voxel_downsample(whole, h)
                t0 = time.perf_counter()
                state = cloud.state()
                state_wall.append((time.perf_counter() - t0) * 1e6)
                target = m.voxel_downsample(np.zeros((0, 4)), h, context=ctx)
                t0 = time.perf_counter()
                target.merge(state)
                merge_wall.append((time.perf_counter() - t0) * 1e6)
        r = {"M": M, "emit_keys_counts_sums_us": spread(emit),
             "merge_phases_us": spread([sum(x.values()) for x in merge]),
             **{"merge_" + p + "_us": spread([x[p] for x in merge]) for p in INSERT_PHASES}}
        if state_wall:
            r["state_wall_with_host_copies_us"], r["merge_wall_with_host_copies_us"] = spread(state_wall), spread(merge_wall)
        result["cases"][f"h={h} records"] = r
        print(f"h {h:5.2f} records of M {M:9d}: the emits {fmt(r['emit_keys_counts_sums_us'])}  merge into an empty cloud "
              f"{fmt(r['merge_phases_us'])}  " + "  ".join(f"{p} {r['merge_' + p + '_us']['median']:9.1f}" for p in INSERT_PHASES) +
              (f"   with host copies: state() {fmt(r['state_wall_with_host_copies_us'])}  merge() {fmt(r['merge_wall_with_host_copies_us'])}"
               if state_wall else ""), flush=True)
        del bufs

    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
