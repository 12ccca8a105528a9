"""Time the density clustering of a voxel cloud (VoxelCloud.clusters; csrc/cluster.hpp) on the config-2 cloud of
tools/bench_normals.py: urban_complex figure_eight, 600 frames x 100 000 synthetic points, pose_slerp, voxelised
at h = 0.05 and h = 0.2, with eps = 2 h and min_points 1 and 10.

    python tools/bench_clusters.py [--frames 600] [--points 100000] [--repeat 3] [--json out.json]

Per voxel size and min_points: M, K, the noise share, and per phase (density, union, label, number, stats;
mc_timing_read_clusters) the event time in ms, voxels/s and table probes/s (a probe = one window cell looked up:
(2R + 1)^3 per voxel in the density phase, the half of them after the centre per core voxel in the union phase,
the whole window per voxel that is not core in the label phase; the steps of a chain are not counted).  Median of
--repeat.  The library is called directly on device buffers, so only K crosses to the host inside a timed call.

In the same process, on the same cloud: the unchanged normals' window phase (mc_voxel_normals at radius = eps
without a cap, so no cap launch), which does the same probes as the density phase — the yardstick.  The density
phase is expected near it and the union phase, with every voxel core, near half of it; both ratios are printed so
that a miss shows.
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
SIZES = (0.05, 0.2)
MIN_POINTS = (1, 10)
PHASES = ("density", "union", "label", "number", "stats")


def main():
    from bench_normals import setup

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx, out = setup(m, args.frames, args.points)
    n = args.frames * args.points
    result = {"frames": args.frames, "points": n, "repeat": args.repeat, "cases": {}}
    print(f"{args.frames} frames x {args.points} points = {n} points; eps = 2 h; median of {args.repeat}")
    lib, handle = ctx.lib, ctx.handle
    for h in SIZES:
        eps = 2 * h
        cloud = ctx.voxel_downsample(out, h)
        M = cloud.n_voxels
        R = int(np.ceil(eps / h))
        window = (2 * R + 1) ** 3
        d_lab, d_den = ctx.device_buffer(max(M, 1) * 4), ctx.device_buffer(max(M, 1) * 4)
        d_nrm = ctx.device_buffer(max(M, 1) * 32)
        # the yardstick: the normals' window phase without a cap (the first call also writes the centroids)
        m._lib.check(lib.mc_voxel_normals(handle, eps, 0, None, d_nrm.ptr, None, None), "normals")
        ctx.read_timing_normals()
        wins = []
        for _ in range(args.repeat):
            ctx.timing(True)
            m._lib.check(lib.mc_voxel_normals(handle, eps, 0, None, d_nrm.ptr, None, None), "normals")
            ctx.timing(False)
            wins.append(ctx.read_timing_normals()["window_ms"])
        win = float(np.median(wins))
        d_nrm.close()
        print(f"h {h:5.2f}  M {M:9d}  R {R}  normals' window phase {win:9.3f} ms  {M * window / (win * 1e-3) / 1e9:6.2f} Gprobe/s",
              flush=True)
        for mp in MIN_POINTS:
            k = ctypes.c_int64(0)
            runs = []
            for rep in range(args.repeat + 1):
                ctx.read_timing_clusters()
                ctx.timing(True)
                m._lib.check(lib.mc_voxel_clusters(handle, eps, mp, 0, d_lab.ptr, d_den.ptr, ctypes.byref(k)), "clusters")
                K = k.value
                d_st = ctx.device_buffer(max(K, 1) * 36)
                b = d_st.ptr.value
                m._lib.check(lib.mc_voxel_cluster_stats(handle, b + 8 * K, b, b + 12 * K, b + 24 * K), "cluster stats")
                ctx.timing(False)
                t = ctx.read_timing_clusters()
                d_st.close()
                if rep:                   # the first call allocates
                    runs.append([t[p + "_ms"] for p in PHASES])
            ms = np.median(np.array(runs), axis=0)
            labels = d_lab.to_host(np.int32, count=M)
            density = d_den.to_host(np.int32, count=M)
            cores = int((density >= mp).sum())
            probes = {"density": M * window, "union": cores * (window - 1) // 2, "label": (M - cores) * window}
            r = {"M": M, "R": R, "K": K, "noise_share": float((labels < 0).mean()), "core_share": cores / max(M, 1),
                 "largest_share": float(np.bincount(labels[labels >= 0]).max() / M) if K else 0.0,
                 "window_ms": win, "all_ms": [list(map(float, x)) for x in runs]}
            for p, v in zip(PHASES, ms):
                r[p + "_ms"] = float(v)
                r[p + "_voxels_per_s"] = M / (v * 1e-3) if v > 0 else None
                if p in probes:
                    r[p + "_probes_per_s"] = probes[p] / (v * 1e-3) if v > 0 else None
            r["density_over_window"] = r["density_ms"] / win
            r["union_over_window"] = r["union_ms"] / win
            result["cases"][f"h={h} min_points={mp}"] = r
            print(f"h {h:5.2f}  min_points {mp:2d}  K {K:8d}  noise {100 * r['noise_share']:6.2f} %  core {100 * r['core_share']:6.2f} %  "
                  f"largest {100 * r['largest_share']:6.2f} %  " + "  ".join(f"{p} {v:9.3f}" for p, v in zip(PHASES, ms)) + " ms  "
                  f"density {r['density_probes_per_s'] / 1e9:6.2f} Gprobe/s  {M / (ms[:4].sum() * 1e-3) / 1e6:7.1f} Mvoxel/s over the four "
                  f"phases  density / window {r['density_over_window']:.2f}  union / window {r['union_over_window']:.2f}", flush=True)
        d_lab.close()
        d_den.close()
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
