"""The ray-march scanner's contract restated in numpy, and the scenes its tests use.

``LiDARSimulator.simulate_scan`` (CSIM:1011-1055) marches every ray in steps
``d_k = np.arange(range_min, range_max, 0.1)[k]`` and, at each sample ``c = origin + direction * d_k``,
takes ``np.linalg.norm(obj[:, :3] - c, axis=1)`` over every object (``_raycast``, CSIM:1108-1146).  The
first step with a point closer than 0.1 decides the hit: the first object in list order with such a
point (empty objects skipped), within it the closest point (lowest index on ties); the hit point is
the sample, the intensity the point's column 3 or 100.  ``march_frame`` finds the same minimum of the
key (k, object, distance, point index) without marching: a point can be close to sample k only inside
the ray's 0.1 tube with its along-ray coordinate within 0.1 of d_k, so it filters (ray, point) pairs
with a widened tube and evaluates the reference's own expressions (numpy's elementwise multiply, add
and ``np.linalg.norm(..., axis=1)``) at the steps around ``(s - range_min) / 0.1`` only.  It also
reports the edge margin, the smallest |distance - 0.1| it evaluated: the device may decide a pair
differently only within rounding of that edge.

``emit_frame`` restates CSIM:1033-1051 (world -> sensor, noise, clip, tag); ``pattern`` / ``directions``
/ ``rotations`` / ``steps_of`` restate the host tables (CSIM:1057-1106, 1121, 1155-1170).  The scene
builders are shared by tests/golden/make_golden_raymarch.py (which runs the reference on them) and
the tests.
"""
from __future__ import annotations

import numpy as np

STEP = 0.1
DEFAULTS = {"fov_horizontal": 70.4, "fov_vertical": 77.2, "range_max": 90.0, "range_min": 0.05,
            "points_per_frame": 10000, "lidar_range_noise": 0.02, "lidar_intensity_noise": 5.0,
            "random_seed": 42}


def cfg_of(config: dict) -> dict:
    return {**DEFAULTS, **config}


def pattern(config: dict) -> list:
    """CSIM:1057-1079, truncated as CSIM:1019 does."""
    c = cfg_of(config)
    angles = []
    n_rings = 16
    ppr = c["points_per_frame"] // n_rings
    for ring in range(n_rings):
        el = (ring / (n_rings - 1) - 0.5) * np.radians(c["fov_vertical"])
        for point in range(ppr):
            az = (point / ppr) * 2 * np.pi + ring * 0.1
            if abs(np.degrees(az)) <= c["fov_horizontal"] / 2:
                angles.append((az, el))
    return angles[:min(c["points_per_frame"], len(angles))]


def directions(config: dict) -> np.ndarray:
    """CSIM:1081-1086 for every ray of the pattern."""
    return np.array([[np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)] for az, el in pattern(config)],
                    dtype=np.float64).reshape(-1, 3)


def steps_of(config: dict) -> np.ndarray:
    c = cfg_of(config)
    return np.arange(c["range_min"], c["range_max"], STEP)


def rotations(orientation) -> tuple:
    """(R, R_inv): CSIM:1090-1105 and CSIM:1155-1170."""
    def mats(r, p, y):
        R_x = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
        R_y = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
        R_z = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
        return R_x, R_y, R_z
    roll, pitch, yaw = orientation
    R_x, R_y, R_z = mats(roll, pitch, yaw)
    R = R_z @ R_y @ R_x
    R_x, R_y, R_z = mats(-roll, -pitch, -yaw)
    return R, R_x @ R_y @ R_z


def flatten(objects) -> tuple:
    """(xyz (N, 3), intensity (N,), object (N,), index in object (N,)) of a scene's non-empty objects."""
    xyz, inten, oid, idx = [], [], [], []
    for k, obj in enumerate(objects):
        a = np.asarray(obj, dtype=np.float64)
        if len(a) == 0:
            continue
        xyz.append(a[:, :3])
        inten.append(a[:, 3] if a.shape[1] > 3 else np.full(len(a), 100.0))
        oid.append(np.full(len(a), k, np.int64))
        idx.append(np.arange(len(a), dtype=np.int64))
    if not xyz:
        return np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(xyz), np.concatenate(inten), np.concatenate(oid), np.concatenate(idx)


def march_frame(origin, orientation, config: dict, objects, flat=None) -> dict:
    """Every ray's first hit for one sensor pose.  Returns step / object / index (n_rays,) int32 (-1:
    miss), hit_point (n_rays, 3) and intensity (n_rays,) (NaN for misses), world_dir (n_rays, 3) and
    edge_margin."""
    origin = np.asarray(origin, dtype=np.float64)
    R, _ = rotations(orientation)
    dirs = directions(config)
    steps = steps_of(config)
    n, K = len(dirs), len(steps)
    W = np.array([R @ d for d in dirs]).reshape(-1, 3)            # CSIM:1106, the reference's own product
    xyz, inten, oid, idx = flatten(objects) if flat is None else flat
    out = {"step": np.full(n, -1, np.int32), "object": np.full(n, -1, np.int32), "index": np.full(n, -1, np.int32),
           "hit_point": np.full((n, 3), np.nan), "intensity": np.full(n, np.nan), "world_dir": W,
           "edge_margin": np.inf}
    if n == 0 or K == 0 or len(xyz) == 0:
        return out
    V = xyz - origin
    r2 = (V * V).sum(axis=1)
    near = np.flatnonzero(r2 <= (steps[-1] + 0.3) ** 2)
    if near.size == 0:
        return out
    S = V[near] @ W.T                                              # along-ray coordinate of every pair
    cand = (r2[near, None] - S * S <= (STEP * (1 + 1e-5)) ** 2) & (S >= steps[0] - 0.2) & (S <= steps[-1] + 0.2)
    margin = np.inf
    for ray in np.flatnonzero(cand.any(axis=0)):
        loc = np.flatnonzero(cand[:, ray])
        pts = near[loc]
        k0 = np.floor((S[loc, ray] - steps[0]) / STEP).astype(np.int64)
        best = None
        for k in range(max(int(k0.min()) - 2, 0), min(int(k0.max()) + 3, K - 1) + 1):
            sel = pts[(k0 - 2 <= k) & (k <= k0 + 3)]
            if sel.size == 0:
                continue
            current = origin + W[ray] * steps[k]                   # CSIM:1122
            dist = np.linalg.norm(xyz[sel] - current, axis=1)      # CSIM:1130
            margin = min(margin, float(np.abs(dist - STEP).min()))
            close = dist < STEP                                    # CSIM:1131
            if not close.any():
                continue
            o = oid[sel][close].min()                              # first object in list order (CSIM:1125, 1141)
            m = close & (oid[sel] == o)
            j = sel[m][np.argmin(dist[m])]                         # CSIM:1134 (scene order = index order)
            best = (k, j, current)
            break
        if best is not None:
            k, j, current = best
            out["step"][ray], out["object"][ray], out["index"][ray] = k, oid[j], idx[j]
            out["hit_point"][ray] = current
            out["intensity"][ray] = inten[j]
    out["edge_margin"] = margin
    return out


def noise_of(rng, n_hits: int, config: dict) -> np.ndarray:
    """(n_hits, 4): the draws of CSIM:1038-1039 for consecutive hits, as consecutive standard normals."""
    c = cfg_of(config)
    g = rng.standard_normal(4 * n_hits).reshape(n_hits, 4)
    return np.column_stack([0 + c["lidar_range_noise"] * g[:, :3], 0 + c["lidar_intensity_noise"] * g[:, 3]])


def emit_frame(march: dict, origin, orientation, config: dict, noise: np.ndarray, timestamp: int) -> dict:
    """CSIM:1033-1051 for the hits of ``march``: rows (H, 5) = x, y, z, clipped intensity, ray index;
    intensity_int, timestamp, ring, tag per hit; tag_margin."""
    c = cfg_of(config)
    origin = np.asarray(origin, dtype=np.float64)
    _, Rinv = rotations(orientation)
    rays = np.flatnonzero(march["step"] >= 0)
    rows = np.zeros((len(rays), 5))
    for h, i in enumerate(rays):
        p = Rinv @ (march["hit_point"][i] - origin)               # CSIM:1152-1171
        p = p + noise[h, :3]
        w = np.clip(march["intensity"][i] + noise[h, 3], 0, 255)
        rows[h] = (p[0], p[1], p[2], w, i)
    norm = np.array([np.linalg.norm(r[:3]) for r in rows]).reshape(-1)
    return {"rows": rows, "intensity_int": rows[:, 3].astype(np.int64), "timestamp": timestamp + rays * 1000,
            "ring": rays % 16, "tag": (norm > c["range_max"] * 0.9).astype(np.int64),
            "tag_margin": float(np.abs(norm - c["range_max"] * 0.9).min()) if len(rows) else np.inf}


# ---- scenes -----------------------------------------------------------------------------------
CFG_A = {"range_max": 12.0}
POSES_A = (np.array([[0.0, 0.0, 1.5], [0.3, 0.1, 1.6], [0.5, -0.2, 1.4]]),
           np.array([[0.02, -0.03, 0.1], [-0.05, 0.04, 0.4], [0.03, 0.02, -0.2]]))
STAMPS_A = (0, 100_000_000, 200_000_000)


def scene_a() -> list:
    """Case A: ground patch (4 columns), an empty object, a wall without intensity (3 columns), a
    pillar with an extra column (5)."""
    rng = np.random.default_rng(11)
    gx, gy = np.meshgrid(np.arange(0.4, 6.0, 0.3), np.arange(-3.0, 6.0, 0.3))
    n = gx.size
    ground = np.column_stack([gx.ravel() + 0.03 * rng.standard_normal(n), gy.ravel() + 0.03 * rng.standard_normal(n),
                              0.02 * rng.standard_normal(n), rng.uniform(10, 250, n)])
    wy, wz = np.meshgrid(np.arange(-1.0, 4.0, 0.15), np.arange(0.0, 1.2, 0.15))
    wall = np.column_stack([np.full(wy.size, 4.0) + 0.01 * rng.standard_normal(wy.size), wy.ravel(), wz.ravel()])
    m = 500
    pillar = np.column_stack([2.5 + 0.15 * rng.standard_normal(m), 1.5 + 0.15 * rng.standard_normal(m),
                              rng.uniform(0.0, 1.2, m), rng.uniform(0, 255, m), rng.uniform(0, 1, m)])
    return [ground, np.zeros((0, 4)), wall, pillar]


CFG_B = {"points_per_frame": 160, "range_max": 6.0}
POSE_B = (np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0]))


def _place(w, s, perp):
    """The point at along-ray coordinate s and distance perp from the ray through the origin along w."""
    u = np.cross(w, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    return w * s + u * perp


def scenes_b() -> list:
    """Case B: two handmade scenes for the 7-ray pattern of points_per_frame = 160, sensor at the
    origin, identity orientation.  Scene 0, one feature per ray: ray 0 two objects close at the same
    step, the later one nearer (the earlier wins); ray 1 a point close at step k and nearer at k + 1
    (step k wins); ray 2 duplicated points with different intensities (the lower index wins); ray 3 a
    point past range_max but within 0.1 of the last sample (a hit); ray 4 a point further past
    range_max (a miss); ray 5 a point behind the sensor (a miss); ray 6 nothing.  Scene 1: one point
    behind the sensor and below range_min, within 0.1 of every ray's first sample (all rays hit at
    step 0)."""
    W = directions(CFG_B)
    d = steps_of(CFG_B)
    assert len(W) == 7
    k = 30
    obj0 = np.array([np.append(_place(W[0], d[k] + 0.04, 0.07), 40.0),
                     np.append(_place(W[1], d[k] + 0.07, 0.05), 60.0),
                     np.append(_place(W[2], d[k] + 0.02, 0.03), 50.0),
                     np.append(_place(W[2], d[k] + 0.02, 0.03), 150.0),
                     np.append(_place(W[3], d[-1] + 0.07, 0.01), 70.0),
                     np.append(_place(W[4], d[-1] + 0.35, 0.0), 80.0),
                     np.append(_place(W[5], -1.0, 0.0), 90.0)])
    obj1 = np.array([np.append(_place(W[0], d[k] + 0.04, 0.03), 200.0)])
    scene1 = [np.zeros((0, 4)), np.array([[-0.02, 0.001, 0.002, 33.0]])]
    return [[obj0, obj1], scene1]


CFG_C = {"range_max": 260.0}
POSE_C = (np.array([0.0, 0.0, 12.0]), np.array([0.0, -0.12, 0.05]))


def scene_c() -> list:
    """Case C: a 0.5 m ground grid, and wall panels facing the sensor at 120, 180 and 250 m (2 600 march
    steps) in the path of every fifth ray (those that miss the ground reach them)."""
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(15.0, 100.0, 0.5), np.arange(-5.0, 45.0, 0.5))
    n = gx.size
    ground = np.column_stack([gx.ravel() + 0.05 * rng.standard_normal(n), gy.ravel() + 0.05 * rng.standard_normal(n),
                              0.03 * rng.standard_normal(n), rng.uniform(10, 250, n)])
    R, _ = rotations(POSE_C[1])
    a, b = np.meshgrid(np.arange(-0.45, 0.46, 0.15), np.arange(-0.45, 0.46, 0.15))
    walls = {120.0: [], 180.0: [], 250.0: []}
    for i, d in enumerate(directions(CFG_C)[::5]):
        w = R @ d
        u = np.cross(w, [0.0, 0.0, 1.0])
        u /= np.linalg.norm(u)
        v = np.cross(w, u)
        dist = (120.0, 180.0, 250.0)[i % 3]
        walls[dist].append(POSE_C[0] + w * (dist + 0.013 * i) + a.reshape(-1, 1) * u + b.reshape(-1, 1) * v)
    near, mid, far = (np.concatenate(walls[k]) for k in (120.0, 180.0, 250.0))
    mid = np.column_stack([mid, rng.uniform(10, 250, len(mid))])
    far = np.column_stack([far, rng.uniform(10, 250, len(far))])
    return [ground, far, near, mid]


CFG_D = {"range_max": 12.0}


def scene_d(n_objects: int = 65, n_points: int = 50_000) -> list:
    """The no-golden case: ``n_objects`` interleaved objects over one ground area, so that a ray's
    candidates come from many objects and from every part of the concatenated scene."""
    rng = np.random.default_rng(23)
    x = rng.uniform(-18.0, 32.0, n_points)
    y = rng.uniform(-22.0, 28.0, n_points)
    z = 0.03 * rng.standard_normal(n_points)
    w = rng.uniform(0, 255, n_points)
    pts = np.column_stack([x, y, z, w])
    cuts = np.sort(rng.choice(np.arange(1, n_points), n_objects - 2, replace=False))
    objs = np.split(pts, cuts)
    objs[7] = objs[7][:, :3]          # one object without an intensity column
    objs.insert(20, np.zeros((0, 4)))  # and an empty one in the middle of the list
    return objs


def poses_d(n_frames: int = 40) -> tuple:
    t = np.linspace(0.0, 1.0, n_frames)
    pos = np.column_stack([8.0 * t, 6.0 * np.sin(2.0 * t), 1.2 + 0.3 * np.cos(3.0 * t)])
    ori = np.column_stack([0.05 * np.sin(5.0 * t), 0.04 * np.cos(4.0 * t), 1.5 * t - 0.3])
    return pos, ori


def golden_frames() -> dict:
    """name -> (config, position, orientation, objects, timestamp) of every frame of
    tests/golden/csim_raymarch.npz; frames of one case share a simulator, in this order."""
    a, b, c = scene_a(), scenes_b(), scene_c()
    out = {f"A{i}": (CFG_A, POSES_A[0][i], POSES_A[1][i], a, STAMPS_A[i]) for i in range(3)}
    out["B0"] = (CFG_B, POSE_B[0], POSE_B[1], b[0], 5_000_000)
    out["B1"] = (CFG_B, POSE_B[0], POSE_B[1], b[1], 5_000_000)
    out["C0"] = (CFG_C, POSE_C[0], POSE_C[1], c, 7_000_000)
    return out


CASES = {"A": ("A0", "A1", "A2"), "B0": ("B0",), "B1": ("B1",), "C": ("C0",)}


def scene_sha(objects) -> str:
    import hashlib
    h = hashlib.sha256()
    for o in objects:
        a = np.ascontiguousarray(o, dtype=np.float64)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()
