"""Time the relative (sensor-frame) SLERP deskew kernel (mc_deskew_relative: k_deskew_points<1, false, false,
RelArgs> in csrc/kernels.hpp) against the global pose_slerp kernel, another instantiation of the same
template.  Stays out of bench.py.

Workload: BASELINE config 2's batch, 600 frames x 100 000 synthetic points (mc_batch_synth,
MC_BATCH_WITH_TIME, frames at 10 Hz over a figure-eight trajectory).

    python tools/bench_relative.py [--frames 600] [--points 100000] [--rounds 12] [--launches 8] [--json out.json]

Three arms run interleaved in one process, their order rotating from round to round (every arm runs
first, second and third equally often): the global kernel twice (A1, A2) and the relative kernel (R,
reference "start").  Each arm's turn is --warm untimed launches of its own, then --launches timed ones;
the time of a launch is its workgroup span (first workgroup start to last workgroup end on the device
clock, mc_timing_read_spans), as the headline's kernel time is.  Reported: the three medians,
R / A (A = both global arms together), and the A/A spread |A1 - A2| / A — the margin: both kernels do
the same per-point work on the same 36 B per point, so a relative kernel slower than the spread is a
finding.  The global arm is what Context.deskew launches when calls repeat (its launch also carries the
next call's prep workgroups); the relative call launches its prep on its own.

Besides: the compose step's time (k_pose_at + k_rel_compose, HIP events) as the difference of the prep
events of calls that rebuild the relative table (alternating reference times) and of calls that find
it cached, and the wall time per call of both paths over --calls calls.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--spin-ms", type=float, default=300.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if 3 * args.launches > 64:
        ap.error("at most 21 timed launches per arm and round (the span pool holds 64)")
    sys.path.insert(0, ROOT)
    m = importlib.import_module("livox-motion-compensation-sim_amd")
    ctx = m.Context(0)
    F = args.frames
    counts = np.full(F, args.points, np.int64)
    n = int(counts.sum())
    sim = m.LiDARMotionSimulator({"duration": max(120.0, F / 10.0), "trajectory_type": "figure_eight", "max_speed": 12.0,
                                  "lidar_fps": 10})
    tr = sim.add_sensor_noise(sim.generate_trajectory())
    times = sim.lidar_times()[:F]
    ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])
    b = ctx.batch(counts, with_time=True)
    b.synth(seed=0, frame_id_base=1000)
    b.set_frame_times(times)
    out = ctx.batch(counts, with_time=True)

    arms = {"A1": lambda: ctx.deskew(b, out, mode="pose_slerp"),
            "A2": lambda: ctx.deskew(b, out, mode="pose_slerp"),
            "R": lambda: ctx.deskew(b, out, mode="pose_slerp", reference="start")}
    # untimed: the relative table, the tuned state of both paths, sustained clocks
    ctx.timing(False)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < args.spin_ms:
        for name in ("A1", "R"):
            for _ in range(10):
                arms[name]()
        ctx.sync()
    ctx.read_timing()
    ctx.read_timing_spans()
    spans = {k: [] for k in arms}
    names = list(arms)
    for r in range(args.rounds):
        order = names[r % 3:] + names[:r % 3]
        if (r // 3) % 2:
            order = order[::-1]
        for name in order:
            for _ in range(args.warm):
                arms[name]()
            ctx.timing(True)
            for _ in range(args.launches):
                arms[name]()
            ctx.timing(False)
        ctx.sync()
        got = ctx.read_timing_spans()
        ctx.read_timing()
        if len(got) != 3 * args.launches:
            raise RuntimeError(f"expected {3 * args.launches} launch spans, got {len(got)}")
        for i, name in enumerate(order):
            spans[name] += got[i * args.launches:(i + 1) * args.launches]
    med = {k: float(np.median(v)) for k, v in spans.items()}
    a_all = float(np.median(spans["A1"] + spans["A2"]))
    result = {"frames": F, "points": n, "rounds": args.rounds, "launches_per_arm_and_round": args.launches,
              "global_us": a_all, "global_arm_us": [med["A1"], med["A2"]], "relative_us": med["R"],
              "relative_over_global": med["R"] / a_all, "aa_spread": abs(med["A1"] - med["A2"]) / a_all,
              "bytes_per_point": 36, "relative_GBps": 36 * n / (med["R"] * 1e-6) / 1e9,
              "global_GBps": 36 * n / (a_all * 1e-6) / 1e9}
    print(f"{F} frames x {args.points} points; launch spans, median of {args.rounds * args.launches} per arm")
    print(f"global   A1 {med['A1']:8.1f} us   A2 {med['A2']:8.1f} us   A {a_all:8.1f} us   A/A spread {100 * result['aa_spread']:.2f} %")
    print(f"relative R  {med['R']:8.1f} us   R / A {result['relative_over_global']:.4f}")

    # the compose step: prep events of calls that rebuild the table against calls that find it cached
    def prep_us(refs):
        for ref in refs[:2]:
            ctx.deskew(b, out, mode="pose_slerp", reference=ref)
        ctx.sync()
        ctx.read_timing()
        ctx.read_timing_spans()
        ctx.timing(True)
        for ref in refs:
            ctx.deskew(b, out, mode="pose_slerp", reference=ref)
        ctx.timing(False)
        ctx.sync()
        t = ctx.read_timing()
        ctx.read_timing_spans()
        return t["prep_ms"] * 1e3 / len(refs)
    cached = prep_us(["start"] * 20)
    rebuilt = prep_us([times + 0.001 * (i % 2) for i in range(20)])
    result.update(prep_cached_us=cached, prep_rebuilt_us=rebuilt, compose_us=rebuilt - cached)
    print(f"prep events per call: table cached {cached:.1f} us, rebuilt {rebuilt:.1f} us -> compose {rebuilt - cached:.1f} us")

    def wall_us(call):
        for _ in range(10):
            call()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e6 / args.calls
    result["wall_per_call_us"] = {"global": wall_us(arms["A1"]), "relative": wall_us(arms["R"])}
    print(f"wall per call over {args.calls} calls: global {result['wall_per_call_us']['global']:.1f} us, "
          f"relative {result['wall_per_call_us']['relative']:.1f} us")
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    for x in (b, out):
        x.close()


if __name__ == "__main__":
    main()
