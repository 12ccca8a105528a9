"""Time the shrinking of a voxel cloud (VoxelCloud.remove / .subtract; csrc/voxel.hpp "taking voxels and points out") on
BASELINE config 2's globally deskewed batch, the batch tools/bench_voxel.py and tools/bench_voxel_insert.py time the
build and the growth on.

    python tools/bench_voxel_remove.py [--frames 600] [--points 100000] [--rounds 5] [--sizes 0.05,0.2,1.0]
                                       [--plane-iterations 200] [--json out.json]

For each voxel size h, --rounds interleaved rounds, every figure the event time of the call's phases
(mc_timing_read_voxel, mc_timing_read_voxel_insert, mc_timing_read_voxel_remove) and its wall time with the call's
synchronisations and host copies; medians with the lowest and highest:

  one frame   on the full cloud, which already holds one copy of a further frame of 100 000 points: that frame inserted
              (arm A1), subtracted (it empties no voxel: the copy stays), inserted again (arm A2, the A/A spread of the
              insert) and subtracted again, the arms alternating in one process
  remove      the one-shot build, then remove(mask) of it, for a random tenth and a random half of the voxels and for
              the inliers of segment_plane(h, --plane-iterations); every round builds the cloud again
  all of it   the one-shot build, then subtract(the whole batch): every voxel empties and leaves

The removal is timed as one phase (the keep flags, the survivors' ids, their records, the table's refill): how it splits
into the compaction and the refill is not measured here.
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
from bench_voxel_insert import BUILD_PHASES, INSERT_PHASES, Drive, fmt, spread, table, timed  # noqa: E402

REMOVE_PHASES = ("validate", "apply", "check", "compact")


def phases_us(t, names):
    return {p: t[p + "_ms"] * 1e3 for p in names}


def summary(rs, names):
    r = {p + "_us": spread([x[p] for x in rs]) for p in (*names, "wall")}
    r["phases_us"] = spread([sum(x[p] for p in names) for x in rs])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="0.05,0.2,1.0")
    ap.add_argument("--plane-iterations", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    sizes = [float(x) for x in args.sizes.split(",")]
    d = Drive(m, args.frames, args.points)
    ctx = d.ctx
    n = args.frames * args.points
    whole = d.deskewed(0, args.frames)
    extra = d.deskewed(args.frames, args.frames + 1, time_of=args.frames - 1)     # a frame the drive has not seen, at its last pose
    result = {"frames": args.frames, "points": n, "rounds": args.rounds, "cases": {}}
    print(f"{args.frames} frames x {args.points} points = {n} points; median (lowest .. highest) of {args.rounds} interleaved rounds; us")

    def build(h):
        cloud, t, wall = timed(ctx, ctx.read_timing_voxel, lambda: ctx.voxel_downsample(whole, h))
        return cloud, {**phases_us(t, BUILD_PHASES), "wall": wall * 1e3}

    for h in sizes:
        cloud = ctx.voxel_downsample(whole, h)                                     # warm-up: the scratch allocation
        M = cloud.n_voxels
        rng = np.random.default_rng(0)
        masks = {"a random tenth": rng.random(M) < 0.1, "a random half": rng.random(M) < 0.5}
        plane = cloud.segment_plane(h, args.plane_iterations)
        masks["the plane's inliers"] = plane.inliers
        cloud.remove(masks["a random tenth"])                                      # warm-up: the removal's scratch

        # one frame in and out of the full cloud
        cloud = ctx.voxel_downsample(whole, h)
        cloud.insert(extra)                                                        # the copy that stays: no subtract empties a voxel
        Mx, slots = cloud.n_voxels, table(ctx)
        arms = {"insert A1": [], "subtract": [], "insert A2": [], "subtract again": []}
        for _ in range(args.rounds):
            for name in arms:
                if name.startswith("insert"):
                    _, t, wall = timed(ctx, ctx.read_timing_voxel_insert, lambda: cloud.insert(extra))
                    arms[name].append({**phases_us(t, INSERT_PHASES), "wall": wall * 1e3})
                else:
                    gone, t, wall = timed(ctx, ctx.read_timing_voxel_remove, lambda: cloud.subtract(extra))
                    assert gone == 0 and t["compact_ms"] == 0.0
                    arms[name].append({**phases_us(t, REMOVE_PHASES), "wall": wall * 1e3})
        assert cloud.n_voxels == Mx and cloud.n_points == n + args.points and table(ctx) == slots
        for name, rs in arms.items():
            names = INSERT_PHASES if name.startswith("insert") else REMOVE_PHASES
            r = summary(rs, names)
            r["M"] = Mx
            result["cases"][f"h={h} one frame, {name}"] = r
            print(f"h {h:5.2f} one frame, {name:14s} M {Mx:9d}  phases {fmt(r['phases_us'])}  wall {fmt(r['wall_us'])}  " +
                  "  ".join(f"{p} {r[p + '_us']['median']:7.1f}" for p in names), flush=True)
        ins = [result["cases"][f"h={h} one frame, insert {a}"]["phases_us"]["median"] for a in ("A1", "A2")]
        sub = result["cases"][f"h={h} one frame, subtract"]["phases_us"]["median"]
        result["cases"][f"h={h} one frame, ratios"] = {"subtract_over_insert_A1": sub / ins[0], "insert_A2_over_A1": ins[1] / ins[0]}
        print(f"h {h:5.2f} one frame: subtract / insert A1 {sub / ins[0]:.3f}   insert A2 / A1 {ins[1] / ins[0]:.3f}", flush=True)

        # whole voxels out, and everything out, against the one-shot build of the same cloud
        runs = {"one-shot": [], **{name: [] for name in masks}, "subtract the whole batch": []}
        for _ in range(args.rounds):
            for name, mask in masks.items():
                cloud, b = build(h)
                runs["one-shot"].append(b)
                gone, t, wall = timed(ctx, ctx.read_timing_voxel_remove, lambda: cloud.remove(mask))
                assert gone == int(np.count_nonzero(mask)) and cloud.n_voxels == M - gone
                runs[name].append({**phases_us(t, REMOVE_PHASES), "wall": wall * 1e3, "gone": gone, "slots": table(ctx)[0]})
            cloud, b = build(h)
            runs["one-shot"].append(b)
            gone, t, wall = timed(ctx, ctx.read_timing_voxel_remove, lambda: cloud.subtract(whole))
            assert gone == M and cloud.n_voxels == 0 and cloud.n_points == 0
            runs["subtract the whole batch"].append({**phases_us(t, REMOVE_PHASES), "wall": wall * 1e3, "gone": gone, "slots": table(ctx)[0]})
        for name, rs in runs.items():
            names = BUILD_PHASES if name == "one-shot" else REMOVE_PHASES
            r = summary(rs, names)
            r["M"] = M
            if name != "one-shot":
                r["gone"], r["slots_after"] = rs[0]["gone"], rs[0]["slots"]
            result["cases"][f"h={h} {name}"] = r
            print(f"h {h:5.2f} {name:24s} M {M:9d} gone {r.get('gone', 0):9d}  phases {fmt(r['phases_us'])}  wall {fmt(r['wall_us'])}  " +
                  "  ".join(f"{p} {r[p + '_us']['median']:9.1f}" for p in names), flush=True)

    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
