"""Drop-in ``LiDARSimulator`` (CSIM:990-1171): the ray-march scanner that produces Path B's frames.

``simulate_scan`` keeps the reference's signature and returns its ``List[LiDARPoint]``; the march of
every ray against every scene point (``_raycast``, CSIM:1108-1146) runs on the GPU in float64
(``k_ray_count`` / ``k_ray_emit``, csrc/raymarch.hpp) and decides every hit as the reference does.
``simulate_lidar_frames`` is the frame loop of ``_simulate_lidar_frames`` (CSIM:2028-2084) with all
frames in one count launch and one emit launch; ``scan_frames`` leaves the same frames on the device
as a float32 ``Batch`` with per-point times, ready for ``Context.deskew(mode="imu")``.

The host computes in numpy exactly what the reference computes in numpy: the scan pattern and its
unit directions, the rotation matrices R and R_inv of every frame, the ``np.arange`` step table, the
``np.interp`` poses and the noise draws (the simulator's own ``RandomState``, consumed in ray order
for hits only).  There is no CPU fallback: without the library every call raises.
"""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_int32, c_int64
from typing import Dict, List

import numpy as np

from ._lib import check, ptr
from .compensator import LiDARPoint
from .runtime import Batch, Context, default_context

# Mid70Specs (CSIM:63-84)
FOV_HORIZONTAL = 70.4
FOV_VERTICAL = 77.2
RANGE_MAX = 90.0
RANGE_MIN = 0.05
FRAME_RATE = 10
POINT_RATE_MAX = 100000
ANGULAR_RES_H = 0.28
STEP_SIZE = 0.1          # _raycast's march step and hit radius (CSIM:1118)


def rotation_pair(orientation) -> tuple:
    """(R, R_inv) of one sensor orientation: R = R_z R_y R_x (CSIM:1090-1105) and
    R_inv = R_x(-roll) R_y(-pitch) R_z(-yaw) (CSIM:1155-1170), the reference's own numpy products."""
    roll, pitch, yaw = orientation
    out = []
    for r, p, y in ((roll, pitch, yaw), (-roll, -pitch, -yaw)):
        R_x = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
        R_y = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
        R_z = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
        out.append((R_z @ R_y @ R_x) if not out else (R_x @ R_y @ R_z))
    return out[0], out[1]


def scene_rows(environment_objects) -> tuple:
    """(counts, rows): the objects' [x, y, z, intensity] float64 rows back to back; an object with 3
    columns carries the reference's intensity 100 (CSIM:1140)."""
    counts, parts = [], []
    for k, obj in enumerate(environment_objects):
        a = np.asarray(obj)
        if len(a) == 0:
            counts.append(0)           # skipped by the reference (CSIM:1126)
            continue
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError(f"environment object {k}: expected (n, >=3) rows, got shape {a.shape}")
        a = a.astype(np.float64, copy=False)
        rows = np.empty((len(a), 4), np.float64)
        rows[:, :3] = a[:, :3]
        rows[:, 3] = a[:, 3] if a.shape[1] > 3 else 100.0
        counts.append(len(a))
        parts.append(rows)
    rows = np.concatenate(parts) if parts else np.zeros((0, 4))
    return np.asarray(counts, np.int64), np.ascontiguousarray(rows)


class LiDARSimulator:
    """GPU-backed drop-in for livox_mid70_complete_simulator.LiDARSimulator."""

    def __init__(self, config: Dict, *, context: Context | None = None):
        self.config = config
        self.rng = np.random.RandomState(config.get("random_seed", 42))
        self.fov_h = config.get("fov_horizontal", FOV_HORIZONTAL)
        self.fov_v = config.get("fov_vertical", FOV_VERTICAL)
        self.range_max = config.get("range_max", RANGE_MAX)
        self.range_min = config.get("range_min", RANGE_MIN)
        self.points_per_frame = config.get("points_per_frame", POINT_RATE_MAX // FRAME_RATE)
        self.angular_resolution = config.get("angular_resolution", ANGULAR_RES_H)
        self.range_noise_std = config.get("lidar_range_noise", 0.02)
        self.intensity_noise_std = config.get("lidar_intensity_noise", 5.0)
        self._context = context

    @property
    def context(self) -> Context:
        if self._context is None:
            self._context = default_context()
        return self._context

    # ---- host tables, as the reference computes them -------------------------------------------
    def _generate_scan_pattern(self) -> list:
        """CSIM:1057-1079."""
        angles = []
        n_rings = 16
        points_per_ring = self.points_per_frame // n_rings
        for ring in range(n_rings):
            elevation = (ring / (n_rings - 1) - 0.5) * np.radians(self.fov_v)
            for point in range(points_per_ring):
                azimuth = (point / points_per_ring) * 2 * np.pi + ring * 0.1
                if abs(np.degrees(azimuth)) <= self.fov_h / 2:
                    angles.append((azimuth, elevation))
        return angles

    def directions(self) -> np.ndarray:
        """(n_rays, 3) sensor-frame unit vectors of the pattern's first min(points_per_frame, len)
        rays (CSIM:1019-1025, 1081-1086)."""
        angles = self._generate_scan_pattern()
        n = min(self.points_per_frame, len(angles))
        d = np.empty((max(n, 0), 3), np.float64)
        for i in range(n):
            az, el = angles[i]
            d[i] = (np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el))
        return d

    def steps(self) -> np.ndarray:
        """The march distances np.arange(range_min, range_max, 0.1) (CSIM:1121)."""
        return np.ascontiguousarray(np.arange(self.range_min, self.range_max, STEP_SIZE), dtype=np.float64)

    # ---- device passes -------------------------------------------------------------------------
    def _set_scene(self, environment_objects):
        ctx = self.context
        counts, rows = scene_rows(environment_objects)
        last = getattr(ctx, "_ray_scene_last", None)
        if (last is not None and np.array_equal(last[0], counts) and last[1].shape == rows.shape
                and np.array_equal(last[1].view(np.uint64), rows.view(np.uint64))):
            return   # the device already holds these exact bytes
        ctx._ray_scene_last = None
        check(ctx.lib.mc_set_ray_scene(ctx.handle, len(counts), ptr(counts, c_int64), ptr(rows, c_double), 4),
              "set_ray_scene")
        ctx._ray_scene_last = (counts, rows)

    def _count(self, positions, orientations, environment_objects):
        """Pass 1 for F poses: returns (counts, R_inv (F, 3, 3), n_rays)."""
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        ori = np.asarray(orientations, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != 3 or ori.shape != pos.shape:
            raise ValueError(f"expected (F, 3) positions and orientations, got {pos.shape} and {ori.shape}")
        F = len(pos)
        self._set_scene(environment_objects)
        R = np.empty((F, 3, 3), np.float64)
        Rinv = np.empty((F, 3, 3), np.float64)
        for f in range(F):
            R[f], Rinv[f] = rotation_pair(ori[f])
        dirs = self.directions()
        steps = self.steps()
        counts = np.zeros(F, np.int64)
        ctx = self.context
        check(ctx.lib.mc_ray_count(ctx.handle, F, ptr(pos, c_double), ptr(R, c_double), len(dirs), ptr(dirs, c_double),
                                   len(steps), ptr(steps, c_double), STEP_SIZE, ptr(counts, c_int64)), "ray_count")
        return counts, Rinv, len(dirs)

    def hits(self, n_frames: int, n_rays: int) -> np.ndarray:
        """The last count's discrete result (n_frames, n_rays, 3) int32: step, object, point index in
        the object, or -1."""
        out = np.full((n_frames * n_rays, 3), -1, np.int32)
        check(self.context.lib.mc_ray_hits(self.context.handle, ptr(out, c_int32)), "ray_hits")
        return out.reshape(n_frames, n_rays, 3)

    def _noise(self, n_hits: int):
        """The four draws of every hit (CSIM:1038-1039): rng.normal(0, s, 3) then rng.normal(0, s_i)
        are consecutive standard_normal values, scaled."""
        if n_hits == 0:
            return None
        g = self.rng.standard_normal(4 * n_hits).reshape(n_hits, 4)
        noise = np.empty((n_hits, 4), np.float64)
        noise[:, :3] = 0 + self.range_noise_std * g[:, :3]
        noise[:, 3] = 0 + self.intensity_noise_std * g[:, 3]
        return noise

    def scan_rows(self, positions, orientations, environment_objects):
        """Both passes for F poses into float64 rows: returns (counts, rows (H, 5)) with rows =
        x, y, z, clipped noisy intensity, ray index; frames back to back."""
        counts, Rinv, _ = self._count(positions, orientations, environment_objects)
        H = int(counts.sum())
        rows = np.empty((H, 5), np.float64)
        noise = self._noise(H)
        ctx = self.context
        check(ctx.lib.mc_ray_emit_f64(ctx.handle, ptr(Rinv, c_double), ptr(noise, c_double), ptr(rows, c_double)),
              "ray_emit_f64")
        return counts, rows

    def _points(self, rows: np.ndarray, timestamp: int) -> List[LiDARPoint]:
        """CSIM:1043-1051 for one frame's rows."""
        x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
        tag = np.sqrt((x * x + y * y) + z * z) > self.range_max * 0.9
        ray = rows[:, 4].astype(np.int64)
        return [LiDARPoint(x=float(r[0]), y=float(r[1]), z=float(r[2]), intensity=int(r[3]),
                           timestamp=timestamp + int(i) * 1000, ring=int(i) % 16, tag=1 if t else 0)
                for r, i, t in zip(rows, ray, tag)]

    # ---- reference signatures --------------------------------------------------------------------
    def simulate_scan(self, sensor_position, sensor_orientation, environment_objects, timestamp: int) -> List[LiDARPoint]:
        """CSIM:1011-1055 for one frame."""
        _, rows = self.scan_rows(np.asarray(sensor_position, np.float64).reshape(1, 3),
                                 np.asarray(sensor_orientation, np.float64).reshape(1, 3), environment_objects)
        return self._points(rows, timestamp)

    @staticmethod
    def frame_poses(trajectory: Dict, mount_z: float = 0.0) -> tuple:
        """CSIM:2033-2057: (frame_times, positions, orientations, timestamps_ns) of every frame."""
        frame_interval = 1.0 / FRAME_RATE
        frame_times = np.arange(0, trajectory["time"][-1], frame_interval)
        F = len(frame_times)
        pos = np.empty((F, 3), np.float64)
        ori = np.empty((F, 3), np.float64)
        for f, t in enumerate(frame_times):
            pos[f] = [np.interp(t, trajectory["time"], trajectory[k]) for k in ("x", "y", "z")]
            ori[f] = [np.interp(t, trajectory["time"], trajectory[k]) for k in ("roll", "pitch", "yaw")]
            pos[f, 2] += mount_z
        stamps = np.array([int(t * 1e9) for t in frame_times], np.int64)
        return frame_times, pos, ori, stamps

    def simulate_lidar_frames(self, trajectory: Dict, environment_objects, mount_z: float = 0.0) -> List[Dict]:
        """CSIM:2028-2084: every frame's simulate_scan in one count launch and one emit launch;
        returns the reference's ``frames_data`` dicts (``mount_z`` = device_info.z, CSIM:2054)."""
        _, pos, ori, stamps = self.frame_poses(trajectory, mount_z)
        counts, rows = self.scan_rows(pos, ori, environment_objects)
        offs = np.concatenate([[0], np.cumsum(counts)])
        frame_interval = 1.0 / FRAME_RATE
        return [{"frame_id": f, "timestamp": int(stamps[f]), "sensor_position": pos[f].copy(),
                 "sensor_orientation": ori[f].copy(),
                 "points": self._points(rows[offs[f]:offs[f + 1]], int(stamps[f])),
                 "frame_duration_ns": int(frame_interval * 1e9)} for f in range(len(stamps))]

    def scan_frames(self, positions, orientations, environment_objects, timestamps, with_pcd_len: bool = False) -> tuple:
        """The frames of F poses as a device ``Batch`` with time (float32 x, y, z, intensity and
        t_ns = 1000 * ray index) whose frame starts are ``timestamps`` (ns): the input of
        ``Context.deskew(batch, mode="imu")``.  Returns (batch, frame_start_ns)."""
        starts = np.ascontiguousarray(np.atleast_1d(timestamps), dtype=np.int64)
        counts, Rinv, _ = self._count(positions, orientations, environment_objects)
        if len(starts) != len(counts):
            raise ValueError(f"one timestamp per frame expected ({len(counts)}), got {len(starts)}")
        out = self._emit_batch(counts, Rinv, with_pcd_len)
        out.set_frame_starts(starts)
        return out, starts

    def _emit_batch(self, counts, Rinv, with_pcd_len: bool = False) -> Batch:
        """Pass 2 of the last count into a new batch with time."""
        ctx = self.context
        out = Batch(ctx, counts, with_time=True, with_pcd_len=with_pcd_len)
        noise = self._noise(int(counts.sum()))
        check(ctx.lib.mc_ray_emit(ctx.handle, out.handle, ptr(Rinv, c_double), ptr(noise, c_double)), "ray_emit")
        return out

    def read_timing(self) -> tuple:
        """(ms, launches) of the scanner's timed regions since the last read (Context.timing(True))."""
        ms, n = c_double(), c_int64()
        check(self.context.lib.mc_timing_read_ray(self.context.handle, ctypes.byref(ms), ctypes.byref(n)),
              "timing_read_ray")
        return ms.value, n.value
