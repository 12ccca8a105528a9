"""Time the plane segmentation of a voxel cloud and the selection of its inliers into a batch
(VoxelCloud.segment_plane, VoxelCloud.select; csrc/plane.hpp) on the config-2 cloud of tools/bench_normals.py:
urban_complex figure_eight, 600 frames x 100 000 synthetic points, pose_slerp, voxelised at h = 0.05 and h = 0.2,
with t = h and K = 1000 hypotheses, with and without the refit.

    python tools/bench_plane.py [--frames 600] [--points 100000] [--iterations 1000] [--repeat 5] [--subset 200000] [--json out.json]

Per voxel size and refine: M, the winner's score, and per phase (compact, sample, score, mask, moments, select;
mc_timing_read_plane) the event time in ms: the median of --repeat with the lowest and highest beside it.  The four
variants (two voxel sizes cannot share a build, so per voxel size: refine off / on) are interleaved, off, on, off,
on, ..., so that a drift of the machine touches both alike.  Rates: point-plane tests per second of the score phase
(K M tests, 7 float64 operations and 32 B of centroid per K tests), bytes per second of the selection (it reads the
mask twice, writes and reads the ids and reads 36 B of record per selected voxel, writes 16 B per selected voxel:
2 M + (8 + 36 + 16) n bytes).  The library is called directly on device buffers; the score table (4 K bytes) and a
few words cross to the host inside a timed call.  The bench cloud is synthetic: its planes are what the synthetic
scanner's noise leaves of them, and the phases' times do not depend on what the winner is.

Beside it, the same definition in NumPy (tests/planes.py's ransac, restated here without the test helpers) on one core
of this box's CPU over a --subset of the voxels (the first of the cloud) and 100 hypotheses, labelled as such.
"""
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
SIZES = (0.05, 0.2)
PHASES = ("compact", "sample", "score", "mask", "moments", "select")
CPU_HYPOTHESES = 100


def cpu_tests_per_s(cent, t, K, seed=0):
    """The score phase in NumPy on one core: K planes through three random voxels each, every voxel tested against
    each, one IEEE operation per line -> (tests per second, best score)."""
    rng = np.random.default_rng(seed)
    at = np.stack([rng.permutation(len(cent))[:3] for _ in range(K)])
    p0, p1, p2 = cent[at[:, 0]], cent[at[:, 1]], cent[at[:, 2]]
    t0 = time.perf_counter()
    e1 = p1 - p0
    e2 = p2 - p0
    n = np.cross(e1, e2)
    l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    d = -((n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
    tau = (t * t) * l2
    best = 0
    for k in range(K):
        s = ((n[k, 0] * cent[:, 0] + n[k, 1] * cent[:, 1]) + n[k, 2] * cent[:, 2]) + d[k]
        best = max(best, int(np.count_nonzero(s * s <= tau[k])))
    return K * len(cent) / (time.perf_counter() - t0), best


def main():
    from bench_normals import setup

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--subset", type=int, default=200_000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx, out = setup(m, args.frames, args.points)
    n = args.frames * args.points
    K = args.iterations
    result = {"frames": args.frames, "points": n, "iterations": K, "repeat": args.repeat, "cases": {}}
    print(f"{args.frames} frames x {args.points} points = {n} points; t = h; K = {K}; median [lowest, highest] of {args.repeat}")
    lib, handle = ctx.lib, ctx.handle
    for h in SIZES:
        cloud = ctx.voxel_downsample(out, h)
        M = cloud.n_voxels
        d_in = ctx.device_buffer(max(M, 1))
        model, cov = np.zeros(4), np.zeros(6)
        samples, stats = np.zeros(3, np.int32), np.zeros(4, np.int64)

        def segment(refine):
            m._lib.check(lib.mc_voxel_plane(handle, h, K, 0, refine, None, d_in.ptr, m._lib.ptr(model, ctypes.c_double),
                                            m._lib.ptr(cov, ctypes.c_double), m._lib.ptr(samples, ctypes.c_int32),
                                            m._lib.ptr(stats, ctypes.c_int64)), "segment_plane")
            n_in = int(stats[2])
            sel = ctx.batch([n_in])
            m._lib.check(lib.mc_voxel_emit_selected(handle, d_in.ptr, sel.handle), "select")
            return n_in

        runs = {0: [], 1: []}
        kept = {}
        for rep in range(args.repeat + 1):
            for refine in (0, 1):
                ctx.read_timing_plane()
                ctx.timing(True)
                n_in = segment(refine)
                ctx.timing(False)
                t = ctx.read_timing_plane()
                kept[refine] = (int(stats[0]), int(stats[1]), n_in, model.copy())
                if rep:                   # the first call allocates (and writes the centroids)
                    runs[refine].append([t[p + "_ms"] for p in PHASES])
        for refine in (0, 1):
            a = np.array(runs[refine])
            med, lo, hi = np.median(a, axis=0), a.min(axis=0), a.max(axis=0)
            it, score, n_in, mdl = kept[refine]
            sel_bytes = 2 * M + (8 + 36 + 16) * n_in
            r = {"M": M, "iteration": it, "score": score, "n_inliers": n_in, "model": mdl.tolist(),
                 "all_ms": [list(map(float, x)) for x in a]}
            for p, v, l, u in zip(PHASES, med, lo, hi):
                r[p + "_ms"] = [float(v), float(l), float(u)]
            i = PHASES.index("score")
            r["score_tests_per_s"] = [K * M / (x * 1e-3) for x in (med[i], hi[i], lo[i])]
            r["score_centroid_bytes_per_s"] = 32 * M * -(-K // m.voxel.plane_score_chunk()) / (med[i] * 1e-3)
            i = PHASES.index("select")
            r["select_bytes_per_s"] = [sel_bytes / (x * 1e-3) for x in (med[i], hi[i], lo[i])]
            r["call_ms"] = float(med[:5].sum())
            result["cases"][f"h={h} refine={refine}"] = r
            print(f"h {h:5.2f}  refine {refine}  M {M:9d}  winner {it:4d}  score {score:9d}  inliers {n_in:9d}  "
                  + "  ".join(f"{p} {v:8.3f} [{l:8.3f}, {u:8.3f}]" for p, v, l, u in zip(PHASES, med, lo, hi)) + " ms  "
                  f"score {r['score_tests_per_s'][0] / 1e12:6.3f} Ttest/s [{r['score_tests_per_s'][1] / 1e12:6.3f}, "
                  f"{r['score_tests_per_s'][2] / 1e12:6.3f}] = {7 * r['score_tests_per_s'][0] / 1e12:6.2f} TFLOP/s float64  "
                  f"select {r['select_bytes_per_s'][0] / 1e9:7.1f} GB/s [{r['select_bytes_per_s'][1] / 1e9:7.1f}, "
                  f"{r['select_bytes_per_s'][2] / 1e9:7.1f}]", flush=True)
        # one core of this box, over the first voxels of the cloud
        sub = min(args.subset, M)
        if sub >= 3:
            cent = cloud.rows()[:sub, :3].copy()
            rate, best = cpu_tests_per_s(cent, h, CPU_HYPOTHESES)
            result["cases"][f"h={h} cpu"] = {"voxels": sub, "hypotheses": CPU_HYPOTHESES, "tests_per_s": rate, "best": best}
            print(f"h {h:5.2f}  NumPy on one CPU core of this box, {sub} voxels x {CPU_HYPOTHESES} hypotheses: "
                  f"{rate / 1e9:6.3f} Gtest/s", flush=True)
        d_in.close()
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
