"""Time the ray-march scanner (LiDARSimulator.simulate_scan on the GPU; csrc/raymarch.hpp).

Workload: 600 frames x 224 rays (the default pattern) along a figure-eight drive over an
EnvironmentGenerator-sized scene built here (a 400 x 400 ground grid = 160 000 points at 0.5 m plus
box and pole obstacles, one object each), range_max 90 (900 march steps).

    python tools/bench_raymarch.py [--frames 600] [--repeat 3] [--json out.json]

Reports the count pass (k_ray_count + k_ray_merge) and the emit pass (k_ray_emit) from HIP events,
(ray, scene point) pair tests per second, and the float64 rate those imply.  A pair test (ray_tube) is
12 float64 vector instructions in the built gfx950 code: 3 subtractions, 2 multiplies, 5 FMAs and 1
compare, i.e. 15 FLOP.  Both are set against the part's vector FP64 peak of 78.6 TFLOP/s (half the
157.3 TFLOP/s vector FP32 rate of MI355X_MICROARCH.md; one FMA per lane and clock on 16 lanes per
SIMD): ``fp64_tflops`` / ``fp64_peak_fraction`` count the 15 FLOP, ``fp64_issue_fraction`` counts the
12 instructions against the 39.3 T lane-instructions/s that peak stands for (what the loop could reach
if every instruction were an FMA).  The exact predicate runs for a vanishing share of the pairs and
is not counted.

    python tools/bench_raymarch.py --reference /path/to/reference

times the reference's own simulate_scan on this CPU instead (no GPU): one frame of 7 rays
(points_per_frame = 160 leaves the pattern that many) on the same scene cut to the
``--ref-ground`` x ``--ref-ground`` ground points nearest the sensor, and scales to 224 rays; the
march costs one np.linalg.norm over every object per step, so seconds per frame grow with the scene.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_PEAK = 78.6e12
FLOP_PER_PAIR = 15
INSTR_PER_PAIR = 12


def build_scene(ground: int = 400, spacing: float = 0.5, seed: int = 0) -> list:
    rng = np.random.default_rng(seed)
    half = ground * spacing / 2
    g = np.arange(ground) * spacing - half
    gx, gy = np.meshgrid(g, g)
    n = gx.size
    objs = [np.column_stack([gx.ravel(), gy.ravel(), 0.02 * rng.standard_normal(n), rng.uniform(20, 80, n)])]
    for _ in range(40):   # boxes: four vertical faces sampled at 0.2 m
        cx, cy = rng.uniform(-half * 0.8, half * 0.8, 2)
        w, d, h = rng.uniform(2, 8), rng.uniform(2, 8), rng.uniform(2, 6)
        u, z = np.meshgrid(np.arange(0, 1, 0.2 / max(w, d)), np.arange(0, h, 0.2))
        u, z = u.ravel(), z.ravel()
        faces = [np.column_stack([cx - w / 2 + u * w, np.full(u.size, cy - d / 2), z]),
                 np.column_stack([cx - w / 2 + u * w, np.full(u.size, cy + d / 2), z]),
                 np.column_stack([np.full(u.size, cx - w / 2), cy - d / 2 + u * d, z]),
                 np.column_stack([np.full(u.size, cx + w / 2), cy - d / 2 + u * d, z])]
        p = np.concatenate(faces)
        objs.append(np.column_stack([p, rng.uniform(50, 200, len(p))]))
    for _ in range(60):   # poles
        cx, cy = rng.uniform(-half * 0.8, half * 0.8, 2)
        z = np.arange(0, 5, 0.1)
        objs.append(np.column_stack([np.full(z.size, cx), np.full(z.size, cy), z, np.full(z.size, 150.0)]))
    return objs


def poses(n_frames: int) -> tuple:
    t = np.linspace(0, 2 * np.pi, n_frames, endpoint=False)
    pos = np.column_stack([60 * np.sin(t), 40 * np.sin(2 * t), np.full(n_frames, 1.8)])
    yaw = np.arctan2(80 * np.cos(2 * t), 60 * np.cos(t))
    ori = np.column_stack([0.02 * np.sin(3 * t), 0.03 * np.cos(2 * t), yaw])
    return pos, ori


def run_gpu(args) -> dict:
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx = m.Context(0, lib_path=args.lib)
    sim = m.LiDARSimulator({"range_max": 90.0}, context=ctx)
    objs = build_scene()
    E = sum(len(o) for o in objs)
    pos, ori = poses(args.frames)
    n_rays = len(sim.directions())
    sim.scan_rows(pos[:8], ori[:8], objs)           # warm-up: scene upload, allocations, first launches
    ctx.timing(True)
    sim.read_timing()
    count_ms, emit_ms, wall = [], [], []
    hits = 0
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        counts, Rinv, _ = sim._count(pos, ori, objs)
        count_ms.append(sim.read_timing()[0])
        batch = sim._emit_batch(counts, Rinv)
        emit_ms.append(sim.read_timing()[0])
        wall.append(time.perf_counter() - t0)
        hits = int(counts.sum())
        batch.close()
    ctx.timing(False)
    pairs = args.frames * n_rays * E
    c = float(np.median(count_ms))
    out = {"frames": args.frames, "rays": n_rays, "scene_points": E, "objects": len(objs), "steps": len(sim.steps()),
           "hits": hits, "count_ms": c, "count_ms_all": count_ms, "emit_ms": float(np.median(emit_ms)),
           "pairs": pairs, "pairs_per_s": pairs / (c * 1e-3), "fp64_tflops": pairs * FLOP_PER_PAIR / (c * 1e-3) / 1e12,
           "fp64_peak_fraction": pairs * FLOP_PER_PAIR / (c * 1e-3) / FP64_PEAK,
           "fp64_issue_fraction": pairs * INSTR_PER_PAIR / (c * 1e-3) / (FP64_PEAK / 2),
           "ms_per_frame": (c + float(np.median(emit_ms))) / args.frames, "wall_s_count_and_emit": float(np.median(wall))}
    return out


def run_reference(args) -> dict:
    sys.dont_write_bytecode = True
    sys.path.insert(0, args.reference)
    import logging
    logging.disable(logging.CRITICAL)
    csim = importlib.import_module("livox_mid70_complete_simulator")
    objs = build_scene()
    pos, ori = poses(600)
    g = objs[0]
    d = np.abs(g[:, :2] - pos[0, :2]).max(axis=1)
    objs[0] = g[d <= args.ref_ground * 0.5 / 2]       # the ground points nearest the sensor
    E = sum(len(o) for o in objs)
    sim = csim.LiDARSimulator({"range_max": 90.0, "points_per_frame": 160})   # a 7-ray pattern
    n_rays = min(160, len(sim._generate_scan_pattern()))
    t0 = time.perf_counter()
    pts = sim.simulate_scan(pos[0], ori[0], objs, 0)
    dt = time.perf_counter() - t0
    return {"reference_rays": n_rays, "reference_scene_points": E, "reference_objects": len(objs), "hits": len(pts),
            "seconds": dt, "seconds_per_ray": dt / n_rays, "seconds_per_frame_224_rays": dt / n_rays * 224}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="another build of libmcdeskew.so (A/B runs)")
    ap.add_argument("--reference", default=None, help="directory of the reference: time its simulate_scan on the CPU")
    ap.add_argument("--ref-ground", type=int, default=100, help="ground points per side kept for the reference run")
    args = ap.parse_args()
    out = run_reference(args) if args.reference else run_gpu(args)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
