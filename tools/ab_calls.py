"""Interleaved A/B of the HOST cost of one mc_deskew call between library builds, in ONE process on ONE
device (GPU box only) — for changes that leave the device code alone (tools/isa_diff.py says "same") and
can only move what a call does on the host before it returns.

Each library gets its own context and the same small batch: a few frames of a few thousand points, so a
step is launch-bound and the host work of the call is not hidden behind the kernel.  A reading is the wall
time per call of `--calls` back-to-back identical Context.deskew calls and one sync at the end; rounds
alternate between the libraries (shuffled arm order, as tools/ab.py), each reading after a few untimed calls.
Where a batch's pages land moves its kernels (tools/ab.py --replicas), and these calls are short enough for
that to show: each library gets `--replicas` independent contexts, created alternately, every one of them
is read, and a library is judged over all its replicas' readings.

    python tools/ab_calls.py --libs build/variants/lib_parent.so,build/variants/lib_new.so

Prints per mode and library the median, min and max reading (us per call; "issue": the loop alone,
before the sync) with each replica's median; --json PATH also writes them to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab import setup  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="comma list of library builds")
    ap.add_argument("--modes", default="pose_slerp,imu,frame")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=6, help="readings per replica and mode (>= 2 rotations)")
    ap.add_argument("--replicas", type=int, default=3, help="independent contexts (allocations) per library")
    ap.add_argument("--json", default=None, help="also write the readings to this file")
    args = ap.parse_args()
    libs = [l for l in args.libs.split(",") if l]
    arms = [(lib, r) for r in range(args.replicas) for lib in libs]   # created alternately
    runs = {arm: setup(arm[0], args) for arm in arms}
    out = {}
    for mode in args.modes.split(","):
        per = {arm: [] for arm in arms}
        issue = {arm: [] for arm in arms}
        order = list(arms)
        rng = random.Random(1)
        for _ in range(args.rounds):
            rng.shuffle(order)
            for arm in order:
                ctx, (bt, bx), bo = runs[arm]
                bi = bx if mode == "frame" else bt
                for _ in range(20):
                    ctx.deskew(bi, bo, mode=mode)
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    ctx.deskew(bi, bo, mode=mode)
                t1 = time.perf_counter()
                ctx.sync()
                per[arm].append((time.perf_counter() - t0) / args.calls * 1e6)
                issue[arm].append((t1 - t0) / args.calls * 1e6)
        for lib in libs:
            v = [x for arm in arms if arm[0] == lib for x in per[arm]]
            iv = [x for arm in arms if arm[0] == lib for x in issue[arm]]
            reps = [statistics.median(per[arm]) for arm in arms if arm[0] == lib]
            name = os.path.basename(lib)
            out[f"{mode}/{name}"] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v),
                                     "issue_median_us": statistics.median(iv), "replica_medians_us": reps, "readings_us": v}
            print(f"{mode:10s} {name:16s} per call: median {statistics.median(v):6.2f} us  min {min(v):6.2f}  max {max(v):6.2f}"
                  f" | issue median {statistics.median(iv):6.2f} | replicas {', '.join(f'{m:.2f}' for m in reps)}"
                  f"  ({args.calls} calls x {len(v)} readings)", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
