"""Time the registration of a scan against a voxel cloud (VoxelCloud.register; csrc/register.hpp) on the config-2 cloud
of tools/bench_normals.py: urban_complex figure_eight, 600 frames x 100 000 synthetic points, pose_slerp, voxelised
at h = 0.2, with max_distance = 2 h (a window of 5^3 cells), the normals of radius 2 h and max_nn = 30.

    python tools/bench_register.py [--frames 600] [--points 100000] [--iterations 5] [--repeat 5] [--json out.json]

Two sources: frame 0 of the deskewed batch alone (one scan against the map) and the whole batch as one rigid body.
Both start from a pose 5 mm and 0.5 mrad off the identity and run exactly --iterations iterations (the tolerances are
zero), so every call does the same work.  Per source and phase (normals, correspond, leaves, tree, solve;
mc_timing_read_register) the time in ms per call: the median of --repeat with the lowest and highest beside it.  The
calls are interleaved, frame, batch, the normals' own call, frame, batch, ..., so that a drift of the machine touches
all alike; the first round allocates and is not counted.  Rates: window cells per second of the correspondence phase
(N (2W + 1)^3 cells per iteration, whether probed or left out as unable to win: the rate the plain walk would need),
beside the table probes per second of the window phase of VoxelCloud.normals (M (2R + 1)^3 probes, none left out)
measured in the same process, and source points per second of a whole iteration.  The library is called directly; per
iteration fewer than 256 x 28 partials cross to the host.  With MCDESKEW_LIB naming another build of the library (one
whose walk leaves nothing out, say) the same command times that build: run the two alternately to compare them.  The
bench cloud is synthetic: what the registration converges to on it says nothing, and how many cells the walk can leave
out depends on how the source lies on the cloud.
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
H = 0.2
MAX_NN = 30
PHASES = ("normals", "correspond", "leaves", "tree", "solve")


def start_pose():
    T = np.eye(4)
    a = 5e-4
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.003, -0.004, 0.0]
    return T


def main():
    from bench_normals import setup

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx, out = setup(m, args.frames, args.points)
    n = args.frames * args.points
    lib, handle = ctx.lib, ctx.handle
    cloud = ctx.voxel_downsample(out, H)
    M = cloud.n_voxels
    W = int(np.ceil(2 * H / H))
    cells = (2 * W + 1) ** 3
    par = m._lib.RegisterParams(2 * H, 2 * H, 0.0, 0.0, (ctypes.c_double * 16)(*start_pose().reshape(-1)), MAX_NN, args.iterations)
    T, hist, stats = np.zeros(16), np.zeros((args.iterations, 8)), np.zeros(4, np.int64)
    d_out, d_cnt = ctx.device_buffer(max(M, 1) * 32), ctx.device_buffer(max(M, 1) * 4)
    sources = {"frame": (0, args.points), "batch": (-1, n)}
    runs = {k: [] for k in sources}
    window = []
    kept = {}
    print(f"{args.frames} frames x {args.points} points = {n} points; h = {H}, M = {M}; max_distance = 2 h ({cells} cells), "
          f"{args.iterations} iterations per call; median [lowest, highest] of {args.repeat}")
    for rep in range(args.repeat + 1):
        for name, (frame, _) in sources.items():
            ctx.read_timing_register()
            ctx.timing(True)
            m._lib.check(lib.mc_voxel_register_batch(handle, out.handle, frame, ctypes.byref(par), m._lib.ptr(T, ctypes.c_double),
                                                     m._lib.ptr(hist, ctypes.c_double), m._lib.ptr(stats, ctypes.c_int64)), "register")
            ctx.timing(False)
            t = ctx.read_timing_register()
            kept[name] = (int(stats[0]), int(stats[1]), int(stats[2]), hist[:, 1].tolist())
            if rep:
                runs[name].append([t[p + "_ms"] for p in PHASES])
        ctx.read_timing_normals()
        ctx.timing(True)
        m._lib.check(lib.mc_voxel_normals(handle, 2 * H, MAX_NN, None, d_out.ptr, d_cnt.ptr, None), "normals")
        ctx.timing(False)
        t = ctx.read_timing_normals()
        if rep:
            window.append(t["window_ms"])
    result = {"frames": args.frames, "points": n, "h": H, "M": M, "iterations": args.iterations, "repeat": args.repeat, "cases": {}}
    R = int(np.ceil(2 * H / H))
    wmed, wlo, whi = float(np.median(window)), min(window), max(window)
    wrate = [M * (2 * R + 1) ** 3 / (x * 1e-3) for x in (wmed, whi, wlo)]
    result["normals_window"] = {"ms": [wmed, wlo, whi], "probes_per_s": wrate}
    print(f"normals window  M {M:9d}  {wmed:9.3f} [{wlo:9.3f}, {whi:9.3f}] ms  {wrate[0] / 1e9:6.2f} Gprobe/s "
          f"[{wrate[1] / 1e9:6.2f}, {wrate[2] / 1e9:6.2f}]")
    for name, (_, count) in sources.items():
        a = np.array(runs[name])
        med, lo, hi = np.median(a, axis=0), a.min(axis=0), a.max(axis=0)
        pairs, its, status, rr = kept[name]
        i = PHASES.index("correspond")
        probes = count * cells * its
        r = {"N": count, "pairs": pairs, "iterations": its, "status": status, "sum_rr": rr, "all_ms": [list(map(float, x)) for x in a]}
        for p, v, l, u in zip(PHASES, med, lo, hi):
            r[p + "_ms"] = [float(v), float(l), float(u)]
        r["correspond_cells_per_s"] = [probes / (x * 1e-3) for x in (med[i], hi[i], lo[i])]
        per_iteration = float(med[1:].sum()) / its
        r["iteration_ms"] = per_iteration
        r["points_per_s"] = count / (per_iteration * 1e-3)
        result["cases"][name] = r
        print(f"{name:6s} N {count:9d}  pairs {pairs:9d}  " + "  ".join(f"{p} {v:9.3f} [{l:9.3f}, {u:9.3f}]" for p, v, l, u in
                                                                        zip(PHASES, med, lo, hi))
              + f" ms  correspond {r['correspond_cells_per_s'][0] / 1e9:6.2f} Gcell/s [{r['correspond_cells_per_s'][1] / 1e9:6.2f}, "
              f"{r['correspond_cells_per_s'][2] / 1e9:6.2f}]  iteration {per_iteration:9.3f} ms = {r['points_per_s'] / 1e6:8.1f} Mpoint/s",
              flush=True)
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
