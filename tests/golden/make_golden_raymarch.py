"""Generate tests/golden/csim_raymarch.npz by running the reference's LiDARSimulator itself.

Run in the build container only (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_raymarch.py

The reference is imported at run time, as make_golden.py does; only inputs and recorded results are
written.  ``simulate_scan`` (CSIM:1011-1055) runs on the scenes of tests/raymarch.py; ``_raycast`` is
wrapped to record each ray's world direction, hit point and intensity, and ``np.linalg.norm`` is
wrapped for the duration to record, per ray, which distance call decided the hit (step and object by
the call's position in the march, the point by the reference's own argmin) and, per case, the edge
margin: the smallest |distance - 0.1| over every (sample, point) pair the reference evaluated.

Cases (one simulator each, seed 42; keys are prefixed with the frame's name):
  A0 A1 A2  default pattern (224 rays), range_max 12, three poses scanned by one simulator, so the
            noise generator carries over; ``A_rng_*`` is its state afterwards.
  B0 B1     points_per_frame 160 (7 rays), the handmade scenes of raymarch.scenes_b.
  C0        range_max 260 (2 600 steps), one pose over a 0.5 m ground grid and walls out to 250 m.
Per frame: world_dir, hit_point (NaN rows for misses), raw_intensity, step / object / index (-1 for
misses), and the LiDARPoint fields x, y, z, intensity, timestamp, ring, tag of the returned list;
edge_margin, tag_margin; scene_sha (sha256 of the scene's float64 bytes, object by object).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import raymarch as RM  # noqa: E402
from make_golden import import_reference  # noqa: E402


class Recorder:
    """np.linalg.norm with a record of the axis=1 calls of the current _raycast."""

    def __init__(self):
        self.orig = np.linalg.norm
        self.calls = 0
        self.last = None
        self.edge = np.inf
        self.tag = np.inf
        self.tag_level = None

    def __call__(self, x, *a, **kw):
        r = self.orig(x, *a, **kw)
        if kw.get("axis") == 1:
            self.calls += 1
            self.last = r
            if r.size:
                self.edge = min(self.edge, float(np.abs(r - RM.STEP).min()))
        elif self.tag_level is not None and np.ndim(x) == 1:
            self.tag = min(self.tag, abs(float(r) - self.tag_level))
        return r


def run_frame(sim, rec, position, orientation, objects, timestamp):
    nonempty = [k for k, o in enumerate(objects) if len(o)]
    rays = []
    inner = sim._raycast

    def raycast(origin, direction, environment_objects):
        rec.calls, rec.last = 0, None
        hit, inten = inner(origin, direction, environment_objects)
        if hit is None:
            rays.append((direction, np.full(3, np.nan), np.nan, -1, -1, -1))
        else:
            c = rec.calls - 1                              # the call that decided the hit
            close = rec.last < RM.STEP
            j = np.flatnonzero(close)[np.argmin(rec.last[close])]
            rays.append((direction, hit, float(inten), c // len(nonempty), nonempty[c % len(nonempty)], int(j)))
        return hit, inten

    sim._raycast = raycast
    rec.tag_level = sim.range_max * 0.9
    try:
        pts = sim.simulate_scan(position, orientation, objects, timestamp)
    finally:
        sim._raycast = inner
        rec.tag_level = None
    out = {"world_dir": np.array([r[0] for r in rays]), "hit_point": np.array([r[1] for r in rays]),
           "raw_intensity": np.array([r[2] for r in rays]), "step": np.array([r[3] for r in rays], np.int32),
           "object": np.array([r[4] for r in rays], np.int32), "index": np.array([r[5] for r in rays], np.int32)}
    for name, dt in (("x", np.float64), ("y", np.float64), ("z", np.float64), ("intensity", np.int64),
                     ("timestamp", np.int64), ("ring", np.int64), ("tag", np.int64)):
        out[name] = np.array([getattr(p, name) for p in pts], dtype=dt)
    return out


def main():
    _, csim = import_reference()
    rec = Recorder()
    out = {}
    np.linalg.norm = rec
    try:
        def case(names, config, poses, scenes, stamps):
            sim = csim.LiDARSimulator(dict(config))
            rec.edge, rec.tag = np.inf, np.inf
            for name, pos, ori, objs, ts in zip(names, poses[0], poses[1], scenes, stamps):
                for k, v in run_frame(sim, rec, pos.copy(), ori.copy(), objs, ts).items():
                    out[f"{name}_{k}"] = v
                out[f"{name}_scene_sha"] = np.array(RM.scene_sha(objs))
                print(name, "rays", len(out[f"{name}_step"]), "hits", int((out[f"{name}_step"] >= 0).sum()), flush=True)
            return sim, rec.edge, rec.tag

        a = RM.scene_a()
        sim, out["A_edge_margin"], out["A_tag_margin"] = case(("A0", "A1", "A2"), RM.CFG_A, RM.POSES_A, [a, a, a],
                                                              RM.STAMPS_A)
        st = sim.rng.get_state()
        out["A_rng_keys"], out["A_rng_pos"] = np.asarray(st[1], np.uint32), np.array(st[2])
        out["A_rng_has_gauss"], out["A_rng_cached"] = np.array(st[3]), np.array(st[4])
        b = RM.scenes_b()
        for i in range(2):   # a simulator per scene
            _, out[f"B{i}_edge_margin"], out[f"B{i}_tag_margin"] = case(
                (f"B{i}",), RM.CFG_B, (RM.POSE_B[0][None], RM.POSE_B[1][None]), [b[i]], (5_000_000,))
        _, out["C_edge_margin"], out["C_tag_margin"] = case(
            ("C0",), RM.CFG_C, (RM.POSE_C[0][None], RM.POSE_C[1][None]), [RM.scene_c()], (7_000_000,))
    finally:
        np.linalg.norm = rec.orig
    path = os.path.join(HERE, "csim_raymarch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in out:
        if k.endswith("margin"):
            print(k, float(out[k]))


if __name__ == "__main__":
    main()
