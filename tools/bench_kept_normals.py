"""Time the normals a voxel cloud keeps across its edits (VoxelCloud.keep_normals; csrc/normals.hpp "kept normals") on
BASELINE config 2's globally deskewed batch: urban_complex figure_eight, 600 frames x 100 000 synthetic points,
pose_slerp — the batch tools/bench_voxel_insert.py grows its clouds from.

    python tools/bench_kept_normals.py [--frames 600] [--points 100000] [--rounds 5] [--sizes 0.05,0.2,1.0] [--json out.json]

For each voxel size h the full cloud is built once and a further frame of 100 000 points (one the drive has not seen, at
its last pose) is the edit.  --rounds interleaved rounds of, in this order and in one process:

  full pass     cloud.normals(2 h, 30): the device time of its phases (mc_timing_read_normals), the baseline beside
                which everything else is read; its code path is not the kept normals'
  kept          keep_normals(), then the frame inserted and subtracted again: for each the device time of the refresh
                phases (mc_timing_read_kept_normals: mark, window, cap, carry), of the edit's own phases, the wall time
                of the call, and |D| = kept.refreshed_last; then one register of the frame (max_iterations 1): the wall
                time and the device time of its normals phase, which is 0 when the kept rows are read
  plain         drop_normals(), and the same insert, subtract and register on the cloud that keeps none
  remove        a random tenth of the voxels removed (the mask already on the device) from a fresh build that keeps
                normals and from one that does not: wall time, the refresh phases, |D|

Medians with the lowest and highest.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_voxel_insert import Drive, fmt, spread, timed  # noqa: E402

KEPT = ("mark", "window", "cap", "carry")


def kept_us(t):
    return sum(t[p + "_ms"] for p in KEPT) * 1e3


def phases_us(t):
    return sum(v for k, v in t.items() if k.endswith("_ms")) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="0.05,0.2,1.0")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    d = Drive(m, args.frames, args.points)
    ctx = d.ctx
    n = args.frames * args.points
    whole = d.deskewed(0, args.frames)
    extra = d.deskewed(args.frames, args.frames + 1, time_of=args.frames - 1)
    result = {"frames": args.frames, "points": n, "rounds": args.rounds, "cases": {}}
    print(f"{args.frames} frames x {args.points} points = {n} points; one frame of {args.points} as the edit; median (lowest .. highest) "
          f"of {args.rounds} interleaved rounds; us")

    def both(read_edit, call):
        """call() timed: (the edit's phases, the refresh phases, wall), all us."""
        ctx.read_timing_kept_normals()
        _, t, wall = timed(ctx, read_edit, call)
        return phases_us(t), ctx.read_timing_kept_normals(), wall * 1e3

    def register_once(cloud, h):
        ctx.read_timing_register()
        _, t, wall = timed(ctx, ctx.read_timing_register, lambda: cloud.register(extra, 2 * h, max_iterations=1, frame=0))
        return t["normals_ms"] * 1e3, wall * 1e3

    for h in [float(x) for x in args.sizes.split(",")]:
        cloud = ctx.voxel_downsample(whole, h)
        cloud.insert(extra)                  # the cloud holds the frame once: inserting it again makes no voxel, taking it out empties none
        M = cloud.n_voxels
        cloud.normals(2 * h, 30)                                                   # warm-up: the scratch allocation
        runs = {k: [] for k in ("full pass", "insert kept refresh", "insert kept edit", "insert kept wall", "insert plain edit",
                                "insert plain wall", "subtract kept refresh", "subtract kept edit", "subtract kept wall",
                                "subtract plain edit", "subtract plain wall", "register kept normals", "register kept wall",
                                "register plain normals", "register plain wall", "D insert", "D subtract")}
        for _ in range(args.rounds):
            _, t, _ = timed(ctx, ctx.read_timing_normals, lambda: ctx.lib.mc_voxel_normals(
                ctx.handle, 2 * h, 30, None, scratch(ctx, M)[0].ptr, scratch(ctx, M)[1].ptr, None))
            runs["full pass"].append(phases_us(t))
            cloud.keep_normals()
            for name, read, call in (("insert", ctx.read_timing_voxel_insert, lambda: cloud.insert(extra)),
                                     ("subtract", ctx.read_timing_voxel_remove, lambda: cloud.subtract(extra))):
                edit, kept, wall = both(read, call)
                runs[name + " kept refresh"].append(kept_us(kept))
                runs[name + " kept edit"].append(edit)
                runs[name + " kept wall"].append(wall)
                runs["D " + name].append(cloud.kept.refreshed_last)
                if name == "insert":
                    nrm, wall = register_once(cloud, h)
                    runs["register kept normals"].append(nrm)
                    runs["register kept wall"].append(wall)
            assert cloud.n_voxels == M and cloud.kept.full_passes >= 1
            cloud.drop_normals()
            for name, read, call in (("insert", ctx.read_timing_voxel_insert, lambda: cloud.insert(extra)),
                                     ("subtract", ctx.read_timing_voxel_remove, lambda: cloud.subtract(extra))):
                edit, _, wall = both(read, call)
                runs[name + " plain edit"].append(edit)
                runs[name + " plain wall"].append(wall)
                if name == "insert":
                    nrm, wall = register_once(cloud, h)
                    runs["register plain normals"].append(nrm)
                    runs["register plain wall"].append(wall)
        r = {k.replace(" ", "_") + ("" if k.startswith("D ") else "_us"): spread(v) for k, v in runs.items()}
        r["M"] = M
        result["cases"][f"h={h} one frame"] = r
        print(f"h {h:5.2f} M {M:9d}  full pass {fmt(r['full_pass_us'])}", flush=True)
        for name in ("insert", "subtract"):
            key = name + "_"
            print(f"    {name:8s} |D| {int(r['D_' + name]['median']):8d}  refresh {fmt(r[key + 'kept_refresh_us'])}  edit phases kept "
                  f"{fmt(r[key + 'kept_edit_us'])} plain {fmt(r[key + 'plain_edit_us'])}  wall kept {fmt(r[key + 'kept_wall_us'])} plain "
                  f"{fmt(r[key + 'plain_wall_us'])}", flush=True)
        print(f"    register normals phase kept {fmt(r['register_kept_normals_us'])} plain {fmt(r['register_plain_normals_us'])}  wall kept "
              f"{fmt(r['register_kept_wall_us'])} plain {fmt(r['register_plain_wall_us'])}", flush=True)

        # a random tenth removed, from a fresh build each time
        mask = np.random.default_rng(10).random(M) < 0.1
        d_mask = ctx.device_buffer(M)
        d_mask.from_host(mask.view(np.uint8))
        rm = {k: [] for k in ("kept wall", "plain wall", "kept refresh", "kept compact", "plain compact", "D")}
        for _ in range(args.rounds):
            for keep in (True, False):
                cloud = ctx.voxel_downsample(whole, h)
                cloud.insert(extra)
                if keep:
                    cloud.keep_normals()
                gone = ctypes.c_int64(0)
                ctx.read_timing_kept_normals()
                rc, t, wall = timed(ctx, ctx.read_timing_voxel_remove, lambda: ctx.lib.mc_voxel_remove(ctx.handle, d_mask.ptr, ctypes.byref(gone)))
                m._lib.check(rc, "remove")
                assert gone.value == int(mask.sum())
                cloud.n_voxels -= gone.value
                which = "kept" if keep else "plain"
                rm[which + " wall"].append(wall * 1e3)
                rm[which + " compact"].append(phases_us(t))
                if keep:
                    rm["kept refresh"].append(kept_us(ctx.read_timing_kept_normals()))
                    rm["D"].append(cloud.kept.refreshed_last)
        r = {k.replace(" ", "_") + ("" if k == "D" else "_us"): spread(v) for k, v in rm.items()}
        r["M"], r["removed"] = M, int(mask.sum())
        result["cases"][f"h={h} remove a tenth"] = r
        print(f"    remove a tenth ({r['removed']} voxels) |D| {int(r['D']['median']):9d}  wall kept {fmt(r['kept_wall_us'])} plain "
              f"{fmt(r['plain_wall_us'])}  refresh {fmt(r['kept_refresh_us'])}  removal phases kept {fmt(r['kept_compact_us'])} plain "
              f"{fmt(r['plain_compact_us'])}", flush=True)
        del d_mask

    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


_scratch = {}


def scratch(ctx, M):
    """Two device buffers for the rows and counts of a full pass over M voxels, made once per size."""
    if _scratch.get("M") != M:
        _scratch.clear()
        _scratch.update(M=M, bufs=(ctx.device_buffer(32 * M), ctx.device_buffer(4 * M)))
    return _scratch["bufs"]


if __name__ == "__main__":
    main()
