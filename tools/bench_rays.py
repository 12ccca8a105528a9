"""Time the rays through a voxel cloud (VoxelCloud.rays; csrc/rays.hpp) on a synthetic scene: a sensor 1.8 m above the
ground driving 40 m through a closed yard of 80 m x 30 m (ground plus four walls), every beam ending on the nearest of
them.  The map is the voxel cloud of the whole drive; the scan walked through it is one frame of the drive, and the
whole drive.

    python tools/bench_rays.py [--frames 600] [--points 100000] [--rounds 3] [--sizes 0.1,0.2,0.5] [--ego] [--json out.json]

--ego: the map also holds one point at every sensor position (the vehicle's own body, dust at the lens), so every ray of
a frame starts in an occupied voxel and all of a frame's rays add to one word: the contended case.  For each voxel size h and guard 0 and 1, --rounds interleaved rounds of: one frame (frame F / 2 of the batch) and the
whole batch through the cloud, and beside them the yardstick, VoxelCloud.nearest of the same source on the same cloud at
max_distance = h (its correspond phase).  Every figure is the event time of the call's phases (mc_timing_read_voxel_rays,
mc_timing_read_register) and its wall time with the call's synchronisation, buffers and host copies; medians with the
lowest and highest.  From the walk phase: rays per second, and cell transitions per second from the call's `steps`.

To compare two builds of the kernel, run the tool once per library with MCDESKEW_LIB set: the two runs are then
separate processes, not interleaved rounds.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_voxel_insert import fmt, spread, timed  # noqa: E402

YARD = (40.0, 15.0)        # the walls at x = +-40 m and y = +-15 m
HEIGHT = 1.8
DRIVE = 40.0               # the sensor moves from x = -20 m to x = +20 m


def scene(frames, points, seed=0):
    """-> (x, y, z float32 (frames * points,), sensor positions (frames, 3) float64): every frame the same `points` beam
    directions (azimuth all round, elevation -26 .. +14 degrees) from its own sensor position."""
    rng = np.random.default_rng(seed)
    az, el = rng.uniform(0.0, 2.0 * np.pi, points), rng.uniform(-0.45, 0.25, points)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)]).astype(np.float32)
    pos = np.zeros((frames, 3))
    pos[:, 0] = np.linspace(-DRIVE / 2, DRIVE / 2, frames) if frames > 1 else 0.0
    pos[:, 2] = HEIGHT
    out = np.empty((3, frames, points), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ground = np.where(d[2] < 0, -HEIGHT / d[2], np.inf).astype(np.float32)
        t_y = ((np.where(d[1] > 0, YARD[1], -YARD[1])) / d[1]).astype(np.float32)        # the sensor drives along y = 0
        for f in range(frames):
            t_x = ((np.where(d[0] > 0, YARD[0], -YARD[0]) - np.float32(pos[f, 0])) / d[0]).astype(np.float32)
            t = np.minimum(np.minimum(t_ground, t_y), t_x)
            for a in range(3):
                out[a, f] = np.float32(pos[f, a]) + t * d[a]
    return out[0].reshape(-1), out[1].reshape(-1), out[2].reshape(-1), pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="0.1,0.2,0.5")
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--ego", action="store_true", help="the map also holds a point at every sensor position: every ray of a "
                    "frame starts in an occupied voxel and adds to its count")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx = m.Context(0)
    F, P = args.frames, args.points
    x, y, z, pos = scene(F, P)
    batch = ctx.batch(np.full(F, P, np.int64))
    batch.upload_columns(x, y, z, np.zeros(F * P, np.float32))
    del x, y, z
    mid = F // 2
    sources = {"one frame": dict(frame=mid, n=P), "the batch": dict(frame=None, n=F * P)}
    result = {"frames": F, "points": F * P, "rounds": args.rounds, "lib": m._lib.LIB_PATH, "ego": args.ego, "cases": {}}
    print(f"{F} frames x {P} points{', the sensor positions in the map' if args.ego else ''}; median (lowest .. highest) of {args.rounds} interleaved rounds; ms", flush=True)
    for h in [float(s) for s in args.sizes.split(",")]:
        cloud = ctx.voxel_downsample(batch, h)
        if args.ego:
            cloud.insert(np.column_stack([pos, np.zeros(F)]))
        M = cloud.n_voxels
        runs = {}
        for r in range(args.rounds + 1):                     # round 0 warms the scratch up and is not kept
            for name, s in sources.items():
                for guard in (0, 1):
                    res, t, wall = timed(ctx, ctx.read_timing_voxel_rays,
                                         lambda: cloud.rays(batch, pos, guard=guard, max_steps=args.max_steps, frame=s["frame"]))
                    assert res.n_rays == s["n"] and int(res.ended.sum()) == s["n"] - res.n_skipped
                    if r:
                        runs.setdefault((name, f"rays guard {guard}"), []).append(
                            dict(device=t["walk_ms"], clear=t["clear_ms"], wall=wall, steps=res.steps, skipped=res.n_skipped,
                                 passed=int(res.passed.sum(dtype=np.int64)), top=int(res.passed.max())))
                    del res
                near, t, wall = timed(ctx, ctx.read_timing_register, lambda: cloud.nearest(batch, h, frame=s["frame"]))
                if r:
                    runs.setdefault((name, "nearest"), []).append(dict(device=t["correspond_ms"], wall=wall, found=int((near.ids >= 0).sum())))
                del near
        for (name, what), rs in runs.items():
            n = sources[name]["n"]
            c = {"M": M, "n": n, "device_ms": spread([q["device"] for q in rs]), "wall_ms": spread([q["wall"] for q in rs])}
            sec = c["device_ms"]["median"] * 1e-3
            c["per_s"] = n / sec
            line = f"h {h:4.2f} M {M:9d} {name:9s} {what:12s} device {fmt(c['device_ms'])}  wall {fmt(c['wall_ms'])}  {n / sec / 1e6:9.1f} M/s"
            if what != "nearest":
                q = rs[0]
                c.update(steps=q["steps"], skipped=q["skipped"], passed=q["passed"], most_passed_voxel=q["top"],
                         clear_ms=spread([v["clear"] for v in rs]), transitions_per_s=q["steps"] / sec)
                line += (f"  {q['steps'] / n:7.1f} steps/ray  {q['steps'] / sec / 1e9:7.2f} G transitions/s  skipped {q['skipped']}"
                         f"  passed {q['passed']} (most in one voxel {q['top']})  clear {c['clear_ms']['median']:.3f}")
            else:
                c["found"] = rs[0]["found"]
            result["cases"][f"h={h} {name}, {what}"] = c
            print(line, flush=True)
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
