"""Time the registration of every frame of a batch in one call (VoxelCloud.register_frames; csrc/register.hpp
k_rg_frames_*) on the setup of tools/bench_register.py: urban_complex figure_eight, 600 frames x 100 000 synthetic
points, pose_slerp, voxelised at h = 0.2, max_distance = 2 h (a window of 5^3 cells), the normals of radius 2 h and
max_nn = 30, from a pose 5 mm and 0.5 mrad off the identity, exactly --iterations iterations (the tolerances are zero).

    python tools/bench_register_frames.py [--frames 600] [--points 100000] [--iterations 5] [--repeat 5] [--sample 8]
                                          [--json out.json]

Arms, interleaved round by round so that a drift of the machine touches all alike (the first round allocates and is
not counted): `frames` and `frames again`, two identical calls of mc_voxel_register_frames (their difference is the
spread between two identical arms); `batch`, mc_voxel_register_batch of the whole batch as one rigid body, which does
the same point work with one pose: the floor to compare with; and `single`, mc_voxel_register_batch of --sample frames
spread over the batch, one call each: what one correction per frame costs without the batched call, scaled to all
frames and labelled as scaled.  Per arm the median of --repeat with the lowest and highest: the event time of every
phase (mc_timing_read_register_frames: normals, step, tree, solve; mc_timing_read_register for the others), the
iteration time (all phases but the normals, per iteration) and the wall time of the call by the host's clock, which
holds the synchronisations and copies the events do not.  The bench cloud is synthetic: what the registrations
converge to on it says nothing."""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
H = 0.2
MAX_NN = 30
FRAMES_PHASES = ("normals", "step", "tree", "solve")
SINGLE_PHASES = ("normals", "correspond", "leaves", "tree", "solve")


def three(values):
    a = np.asarray(values, np.float64)
    return [float(np.median(a, axis=0)), float(a.min(axis=0)), float(a.max(axis=0))]


def main():
    from bench_normals import setup
    from bench_register import start_pose

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx, out = setup(m, args.frames, args.points)
    F, K = args.frames, args.iterations
    n = F * args.points
    lib, handle = ctx.lib, ctx.handle
    P, cd, ci = m._lib.ptr, ctypes.c_double, ctypes.c_int64
    cloud = ctx.voxel_downsample(out, H)
    M = cloud.n_voxels
    par = m._lib.RegisterParams(2 * H, 2 * H, 0.0, 0.0, (cd * 16)(*start_pose().reshape(-1)), MAX_NN, K)
    Ts, hists, statss = np.zeros((F, 16)), np.zeros((F, K, 8)), np.zeros((F, 4), np.int64)
    T, hist, stats = np.zeros(16), np.zeros((K, 8)), np.zeros(4, np.int64)
    sample = sorted({int(f) for f in np.linspace(0, F - 1, min(args.sample, F))})

    def frames_call():
        m._lib.check(lib.mc_voxel_register_frames(handle, out.handle, ctypes.byref(par), None, P(Ts, cd), P(hists, cd), P(statss, ci)),
                     "register_frames")

    def batch_call(frame):
        m._lib.check(lib.mc_voxel_register_batch(handle, out.handle, frame, ctypes.byref(par), P(T, cd), P(hist, cd), P(stats, ci)),
                     "register")

    def timed(call, read, phases):
        read()
        ctx.timing(True)
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        ctx.timing(False)
        t = read()
        return [t[p + "_ms"] for p in phases] + [wall]

    print(f"{F} frames x {args.points} points = {n} points; h = {H}, M = {M}; max_distance = 2 h, {K} iterations per call; "
          f"median [lowest, highest] of {args.repeat}; single: frames {sample}")
    runs = {"frames": [], "frames again": [], "batch": [], "single": []}
    for rep in range(args.repeat + 1):
        got = {"frames": timed(frames_call, ctx.read_timing_register_frames, FRAMES_PHASES)}
        kept = (statss[:, 0].sum(), statss[:, 1].tolist(), statss[:, 2].tolist())
        got["batch"] = timed(lambda: batch_call(-1), ctx.read_timing_register, SINGLE_PHASES)
        got["frames again"] = timed(frames_call, ctx.read_timing_register_frames, FRAMES_PHASES)
        got["single"] = np.sum([timed(lambda f=f: batch_call(f), ctx.read_timing_register, SINGLE_PHASES) for f in sample], axis=0).tolist()
        if rep:
            for k, v in got.items():
                runs[k].append(v)
    short = int(sum(1 for k in kept[1] if k != K))
    if short:
        print(f"note: {short} of {F} frames ended before iteration {K} (statuses {sorted(set(kept[2]))}): they did less work")
    result = {"frames": F, "points": n, "h": H, "M": M, "iterations": K, "repeat": args.repeat, "sample": sample,
              "pairs": int(kept[0]), "frames_ended_early": short, "arms": {}}
    for name, rows in runs.items():
        a = np.array(rows)
        phases = FRAMES_PHASES if name.startswith("frames") else SINGLE_PHASES
        r = {p + "_ms": three(a[:, i]) for i, p in enumerate(phases)}
        calls = len(sample) if name == "single" else 1
        r["iteration_ms"] = three(a[:, 1:-1].sum(axis=1) / (K * calls))
        r["wall_ms"] = three(a[:, -1])
        r["wall_without_normals_ms"] = three(a[:, -1] - a[:, 0])
        r["all_ms"] = a.tolist()
        result["arms"][name] = r
        print(f"{name:13s} " + "  ".join(f"{p} {r[p + '_ms'][0]:9.3f} [{r[p + '_ms'][1]:9.3f}, {r[p + '_ms'][2]:9.3f}]" for p in phases)
              + f" ms  iteration {r['iteration_ms'][0]:8.3f} [{r['iteration_ms'][1]:8.3f}, {r['iteration_ms'][2]:8.3f}] ms"
              + f"  wall {r['wall_ms'][0]:10.3f} [{r['wall_ms'][1]:10.3f}, {r['wall_ms'][2]:10.3f}] ms", flush=True)
    arms = result["arms"]
    scale = F / len(sample)
    result["frames_over_batch_iteration"] = arms["frames"]["iteration_ms"][0] / arms["batch"]["iteration_ms"][0]
    result["identical_arms_spread"] = abs(arms["frames"]["iteration_ms"][0] - arms["frames again"]["iteration_ms"][0]) / arms["frames"]["iteration_ms"][0]
    result["single_scaled_wall_ms"] = arms["single"]["wall_ms"][0] * scale
    result["single_scaled_wall_without_normals_ms"] = arms["single"]["wall_without_normals_ms"][0] * scale
    print(f"register_frames iteration / whole-batch iteration: {result['frames_over_batch_iteration']:.3f}; two identical arms differ "
          f"by {100 * result['identical_arms_spread']:.2f} %")
    print(f"one call per frame, scaled from {len(sample)} to {F} frames: {result['single_scaled_wall_ms'] / 1e3:.2f} s wall with the "
          f"normals, {result['single_scaled_wall_without_normals_ms'] / 1e3:.2f} s without; register_frames: "
          f"{arms['frames']['wall_ms'][0] / 1e3:.3f} s wall")
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
