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

The second half holds what no golden covers, all decided by ``march_frame``: ``edge_scene`` /
``tie_scene`` (points within one coordinate ulp of the hit radius or of each other's distance, found
by bisection on the reference's predicate), numpy / ``fractions.Fraction`` emulations of wrong
arithmetic (``predicate_mutations``) that show these scenes notice it, scenes sized around the LDS
tile, the 256-ray workgroup and the 256-point block, and the C-ABI calls the GPU tests share.
"""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_int32, c_int64

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


def march_frame(origin, orientation, config: dict, objects, flat=None, dirs=None, steps=None) -> dict:
    """Every ray's first hit for one sensor pose.  Returns step / object / index (n_rays,) int32 (-1:
    miss), hit_point (n_rays, 3) and intensity (n_rays,) (NaN for misses), world_dir (n_rays, 3) and
    edge_margin.  ``dirs`` / ``steps`` replace the config's direction and step tables (the C ABI takes
    both as arguments)."""
    origin = np.asarray(origin, dtype=np.float64)
    R, _ = rotations(orientation)
    dirs = directions(config) if dirs is None else np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    steps = steps_of(config) if steps is None else np.asarray(steps, dtype=np.float64)
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


# ---- decision-edge scenes ------------------------------------------------------------------------
# All of them use R = R_inv = identity (R @ d is d exactly in any summation order, so the expected
# decisions rest on nothing BLAS-dependent) and put the variety into an explicit direction table.
IDENTITY = np.zeros(3)
EDGE_ORIGINS = ((0.0, 0.0, 0.0), (3.7, -2.1, 1.45), (5e5, 4.43e6, 120.0))
TIE_ORIGIN = (3.7, -2.1, 1.45)     # not the zero vector: fma(w, d, 0) is the plain product
_I64_MIN = np.iinfo(np.int64).min


def grid_directions() -> np.ndarray:
    """288 unit vectors on a 24 x 12 azimuth / elevation grid over +-1.05 x +-0.45 rad; neighbours are
    at least 0.08 rad apart (azimuth pitch 0.0913 * cos(0.45), elevation pitch 0.0818)."""
    az, el = np.meshgrid(np.linspace(-1.05, 1.05, 24), np.linspace(-0.45, 0.45, 12), indexing="ij")
    az, el = az.ravel(), el.ravel()
    d = np.column_stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1)[:, None])


def grid_steps() -> np.ndarray:
    return np.ascontiguousarray(steps_of({"range_max": 12.0}))


def _ordered(x) -> np.ndarray:
    """float64 <-> int64 keys that order as the doubles do (an involution on the bit patterns)."""
    i = np.ascontiguousarray(x).view(np.int64)
    return np.where(i >= 0, i, _I64_MIN - i)


def _doubles(key) -> np.ndarray:
    return np.ascontiguousarray(_ordered(np.ascontiguousarray(key, dtype=np.int64).view(np.float64))).view(np.float64)


def bisect_adjacent(pred, P, j, x_true, x_false) -> tuple:
    """For every row of P (N, 3), the two adjacent doubles of coordinate j[i] between x_true[i] (where
    ``pred`` holds) and x_false[i] (where it does not) that straddle ``pred``: returns (P_true, P_false).
    ``pred`` maps (N, 3) points to N booleans and is monotone in that coordinate (every operation in it
    is correctly rounded)."""
    rows = np.arange(len(P))

    def at(key):
        Q = P.copy()
        Q[rows, j] = _doubles(key)
        return Q
    lo, hi = _ordered(np.asarray(x_true, np.float64)), _ordered(np.asarray(x_false, np.float64))
    assert pred(at(lo)).all() and not pred(at(hi)).any()
    for _ in range(70):
        if (np.abs(hi - lo) <= 1).all():
            break
        mid = lo + (hi - lo) // 2
        mid = np.where(np.abs(hi - lo) <= 1, lo, mid)
        t = pred(at(mid))
        lo, hi = np.where(t, mid, lo), np.where(t, hi, mid)
    assert (np.abs(hi - lo) == 1).all()
    return at(lo), at(hi)


def _frames_of(D) -> tuple:
    u = np.cross(D, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u, np.cross(D, u)


def _around(origin, D, w, along, perp, theta) -> np.ndarray:
    """origin + D (w + along) + perp (cos theta u + sin theta v) per row."""
    u, v = _frames_of(D)
    return origin + D * (w + along)[:, None] + perp[:, None] * (np.cos(theta)[:, None] * u + np.sin(theta)[:, None] * v)


def _straddle(pred, C, P):
    """bisect_adjacent on each point's coordinate with the largest |p - c|, between 0.9 and 1.1 of it."""
    rows = np.arange(len(P))
    j = np.abs(P - C).argmax(axis=1)
    x0 = C[rows, j]
    dx = P[rows, j] - x0
    return bisect_adjacent(pred, P, j, x0 + 0.9 * dx, x0 + 1.1 * dx)


def edge_scene(origin, seed: int) -> dict:
    """Per ray of grid_directions() two points within one coordinate ulp of the 0.1 hit radius:
    ``p_out`` just outside it at step k1 and ``p_in`` just inside it at step k2 >= k1 + 6 (k in 30...110),
    adjacent doubles found by bisection on the reference's own predicate.  The expected result of ray r
    is (k2[r], point scene_in[r]); a device that accepts p_out reports k1, one that rejects p_in a miss.
    Returns origin, dirs, steps, objects, k1, k2, scene_out, scene_in (scene indices), p_out, p_in,
    along (the points' along-ray offsets from their samples) and d_out, d_in (their distances)."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, dtype=np.float64)
    D, steps = grid_directions(), grid_steps()
    n = len(D)
    k1 = rng.integers(30, 105, n)
    k2 = rng.integers(k1 + 6, 111)
    pts, dist, along = [], [], []
    for k in (k1, k2):
        a = rng.uniform(-0.04, 0.04, n)
        C = origin + D * steps[k][:, None]                              # CSIM:1122, as march_frame forms it
        P = _around(origin, D, steps[k], a, np.sqrt(0.01 - a * a), rng.uniform(0, 2 * np.pi, n))
        pred = lambda Q, C=C: np.linalg.norm(Q - C, axis=1) < STEP      # CSIM:1130-1131
        inside, outside = _straddle(pred, C, P)
        pts.append(outside if k is k1 else inside)
        dist.append(np.linalg.norm(pts[-1] - C, axis=1))
        along.append(a)
    perm = rng.permutation(2 * n)
    rows = np.zeros((2 * n, 4))
    rows[perm, :3] = np.concatenate(pts)
    rows[:, 3] = rng.uniform(0, 255, 2 * n)
    return {"origin": origin, "dirs": D, "steps": steps, "objects": [rows[:200], np.zeros((0, 4)), rows[200:]],
            "k1": k1, "k2": k2, "scene_out": perm[:n], "scene_in": perm[n:], "p_out": pts[0], "p_in": pts[1],
            "along": along, "d_out": dist[0], "d_in": dist[1]}


TIE_OBJECT_POINTS = 1152      # 8 rays' A and B in the first and last 64 slots: >= 1024 indices (two LDS tiles) apart


def tie_scene(seed: int) -> dict:
    """Per ray of grid_directions() two points A and B of one object (one object per 8 rays), both
    clearly inside the hit radius (0.03...0.07) of one step's sample and of no earlier one.  For 256 rays B
    is one of the two adjacent doubles that straddle dist_B < dist_A ("just nearer" for half of them),
    for 32 rays B has A's coordinates and another intensity; B has the lower scene index for half of
    each kind.  A and B are at least 1024 scene indices apart; filler points behind the sensor bring
    every object to TIE_OBJECT_POINTS.  (A and B must share an object for the key's distance to be
    compared and an object's points are contiguous, so 36 objects of more than 1024 points make this
    scene 41 472 points, not 8 192.)  Returns origin, dirs, steps, objects, k, scene_a, scene_b, A, B,
    d_a, d_b, duplicate, nearer, b_low and winner (the designed scene index)."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(TIE_ORIGIN, dtype=np.float64)
    D, steps = grid_directions(), grid_steps()
    n = len(D)
    k = rng.integers(30, 111, n)
    C = origin + D * steps[k][:, None]
    kind = rng.permutation(n)
    duplicate = kind < 32
    b_low = kind % 2 == 0
    nearer = (kind // 2) % 2 == 0
    r = rng.uniform(0.03, 0.07, n)
    pts = []
    for _ in range(2):          # the along-ray offset is positive: the sample before is farther than 0.1
        a = rng.uniform(0.005, 0.025, n)
        pts.append(_around(origin, D, steps[k], a, np.sqrt(r * r - a * a), rng.uniform(0, 2 * np.pi, n)))
    A, B = pts
    d_a = np.linalg.norm(A - C, axis=1)
    pred = lambda Q: np.linalg.norm(Q - C, axis=1) < d_a
    B_near, B_far = _straddle(pred, C, B)
    B = np.where(duplicate[:, None], A, np.where(nearer[:, None], B_near, B_far))
    d_b = np.linalg.norm(B - C, axis=1)
    n_obj = n // 8
    low = np.concatenate([rng.permutation(64)[:8] for _ in range(n_obj)])
    high = np.concatenate([TIE_OBJECT_POINTS - 64 + rng.permutation(64)[:8] for _ in range(n_obj)])
    base = TIE_OBJECT_POINTS * (np.arange(n) // 8)
    scene_b = base + np.where(b_low, low, high)
    scene_a = base + np.where(b_low, high, low)
    E = TIE_OBJECT_POINTS * n_obj
    rows = np.column_stack([origin[0] + rng.uniform(-6.0, -1.0, E), origin[1] + rng.uniform(-3.0, 3.0, E),
                            origin[2] + rng.uniform(-3.0, 3.0, E), rng.uniform(0, 255, E)])
    filler = np.ones(E, bool)
    filler[scene_a] = filler[scene_b] = False
    rows[scene_a, :3], rows[scene_b, :3] = A, B
    lower = np.minimum(scene_a, scene_b)
    winner = np.where(duplicate | (d_a == d_b), lower, np.where(d_b < d_a, scene_b, scene_a))
    return {"origin": origin, "dirs": D, "steps": steps, "objects": np.split(rows, n_obj), "k": k,
            "scene_a": scene_a, "scene_b": scene_b, "A": A, "B": B, "d_a": d_a, "d_b": d_b, "duplicate": duplicate,
            "nearer": nearer, "b_low": b_low, "winner": winner, "filler": filler}


def march_scene(scene: dict) -> dict:
    """march_frame of an edge / tie scene, with its flattened scene for scene-index lookups."""
    flat = flatten(scene["objects"])
    m = march_frame(scene["origin"], IDENTITY, {}, scene["objects"], flat, dirs=scene["dirs"], steps=scene["steps"])
    starts = np.concatenate([[0], np.cumsum([len(o) for o in scene["objects"]])])
    m["scene_index"] = np.where(m["step"] >= 0, starts[np.maximum(m["object"], 0)] + m["index"], -1)
    return m


# ---- wrong arithmetic, emulated --------------------------------------------------------------------
def _fma(a, b, c) -> np.ndarray:
    """fma(a, b, c) elementwise: the exact rational result, rounded once (Fraction -> float)."""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(a, b, c)
    out = [float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())]
    return np.array(out, dtype=np.float64).reshape(a.shape)


def pair_distance(origin, D, w, P, sample: str = "plain", squares: str = "plain") -> np.ndarray:
    """The distance of point P[i] from the sample origin + D[i] * w[i].  "plain" is the reference's
    arithmetic (a multiply, an add, np.linalg.norm); sample="fma" forms the sample as fma(w, d, o),
    squares="fma" the sum of squares as fma(dz, dz, fma(dy, dy, dx * dx))."""
    C = origin + D * w[:, None] if sample == "plain" else _fma(D, w[:, None], np.asarray(origin, np.float64)[None, :])
    if squares == "plain":
        return np.linalg.norm(P - C, axis=1)
    d = P - C
    return np.sqrt(_fma(d[:, 2], d[:, 2], _fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0])))


def predicate_mutations() -> dict:
    """name -> keyword sets of decide_edges / decide_ties, each one wrong arithmetic a kernel could
    have; "radius" is 0.1 off by 1e-13 relative, either way."""
    return {"fma_sample": [{"sample": "fma"}], "fma_squares": [{"squares": "fma"}],
            "radius": [{"radius": float(np.nextafter(STEP * (1 + 1e-13), np.inf))},
                       {"radius": float(np.nextafter(STEP * (1 - 1e-13), -np.inf))}]}


def decide_edges(scene: dict, sample: str = "plain", squares: str = "plain", radius: float = STEP) -> np.ndarray:
    """(n_rays, 2) step and scene index per ray of an edge scene from its two designed pairs alone."""
    o, D, s = scene["origin"], scene["dirs"], scene["steps"]
    out = pair_distance(o, D, s[scene["k1"]], scene["p_out"], sample, squares) < radius
    inn = pair_distance(o, D, s[scene["k2"]], scene["p_in"], sample, squares) < radius
    return np.column_stack([np.where(out, scene["k1"], np.where(inn, scene["k2"], -1)),
                            np.where(out, scene["scene_out"], np.where(inn, scene["scene_in"], -1))])


def decide_ties(scene: dict, sample: str = "plain", squares: str = "plain") -> np.ndarray:
    """(n_rays,) winning scene index per ray of a tie scene from A and B alone."""
    o, D, w = scene["origin"], scene["dirs"], scene["steps"][scene["k"]]
    d_a = pair_distance(o, D, w, scene["A"], sample, squares)
    d_b = pair_distance(o, D, w, scene["B"], sample, squares)
    b = (d_b < d_a) | ((d_b == d_a) & (scene["scene_b"] < scene["scene_a"]))
    return np.where(b, scene["scene_b"], scene["scene_a"])


EDGE_SEED = 7            # the seeds of the scenes the tests run: tests/test_raymarch_cpu.py asserts that
TIE_SEEDS = (1, 2)       # every emulated mutation changes at least 5 of their rays


# ---- sizes around the LDS tile, the 256-ray group and the 256-point block ---------------------------
TILE_SIZES = (1, 511, 512, 513, 1024, 1025)


def tile_scene(E: int) -> list:
    """E points for case B's 7-ray pattern (sensor at the origin, identity): ray 1 hits the scene's
    first point, ray 5 its last one (E = 1: the only point); the rest is filler behind the sensor.  Two
    objects, split in the middle."""
    rng = np.random.default_rng(1000 + E)
    W, d = directions(CFG_B), steps_of(CFG_B)
    rows = np.column_stack([rng.uniform(-5.0, -1.0, E), rng.uniform(-2.0, 2.0, E), rng.uniform(-2.0, 2.0, E),
                            rng.uniform(0, 255, E)])
    rows[0, :3] = _place(W[1], d[20] + 0.04, 0.03)
    if E > 1:
        rows[E - 1, :3] = _place(W[5], d[41] + 0.02, 0.05)
    return [rows[:E // 2], rows[E // 2:]]


RAY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
COUNT_ORIGINS = np.array([[0.0, 0.0, 0.0], [40.0, -7.0, 1.5], [-35.0, 60.0, 0.8]])


def count_scene(n_rays: int) -> tuple:
    """(dirs, steps, objects): the first n_rays of the tiled grid table, three frames at COUNT_ORIGINS
    over one scene: per frame about 60 % of the rays get one point on the ray, 0.03 past a sample at 3-11 m
    (one object per frame, shuffled)."""
    rng = np.random.default_rng(2000 + n_rays)
    D, steps = np.ascontiguousarray(np.resize(grid_directions(), (n_rays, 3))), grid_steps()
    objects = []
    for f, o in enumerate(COUNT_ORIGINS):
        sel = rng.random(n_rays) < 0.6
        sel[f % n_rays] = True
        k = rng.integers(30, 111, int(sel.sum()))
        pts = o + D[sel] * (steps[k] + 0.03)[:, None]
        objects.append(rng.permutation(np.column_stack([pts, rng.uniform(0, 255, len(pts))])))
    return D, steps, objects


CFG_BLOCK = {"points_per_frame": 20000, "range_max": 90}
BLOCK_HITS = (257, 0, 441, 1, 256, 255)
BLOCK_ORIGINS = np.array([[3.0 + f, 400.0 * f, 1.5 + 0.1 * f] for f in range(6)])


def block_scene() -> tuple:
    """(objects, rays): six frames of the 441-ray pattern (points_per_frame = 20000) at BLOCK_ORIGINS,
    400 m apart, over one scene; frame f hits exactly its chosen BLOCK_HITS[f] rays (``rays[f]``, sorted):
    one point per chosen ray on the ray, 0.03 past a sample at 56-64 m.  One object per frame (an empty
    one for the frame without hits), shuffled."""
    rng = np.random.default_rng(3000)
    D, steps = directions(CFG_BLOCK), steps_of(CFG_BLOCK)
    assert len(D) == 441 and len(steps) == 900
    objects, rays = [], []
    for o, n in zip(BLOCK_ORIGINS, BLOCK_HITS):
        sel = np.sort(rng.choice(len(D), n, replace=False))
        k = rng.integers(560, 641, n)
        pts = o + D[sel] * (steps[k] + 0.03)[:, None]
        objects.append(rng.permutation(np.column_stack([pts, rng.uniform(0, 255, n)])))
        rays.append(sel)
    return objects, rays


# ---- the C ABI from the tests -----------------------------------------------------------------------
def ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def abi_count(mc, ctx, cfg, positions, orientations, objects, set_scene=True, dirs=None, steps=None):
    """mc_set_ray_scene + mc_ray_count + mc_ray_hits; returns (counts, hits (F, n, 3), R_inv).  ``dirs``
    / ``steps`` replace the config's tables."""
    lib = ctx.lib
    ctx._ray_scene_last = None      # the Python layer's upload cache does not see this direct call
    if set_scene:
        counts, rows = mc.raymarch.scene_rows(objects)
        mc._lib.check(lib.mc_set_ray_scene(ctx.handle, len(counts), ptr(counts, c_int64), ptr(rows, c_double), 4))
    pos = np.ascontiguousarray(np.atleast_2d(positions), dtype=np.float64)
    rot = [rotations(o) for o in np.atleast_2d(orientations)]
    R = np.ascontiguousarray([r[0] for r in rot])
    Rinv = np.ascontiguousarray([r[1] for r in rot])
    dirs = np.ascontiguousarray(directions(cfg) if dirs is None else dirs, dtype=np.float64)
    steps = np.ascontiguousarray(steps_of(cfg) if steps is None else steps, dtype=np.float64)
    n = np.zeros(len(pos), np.int64)
    mc._lib.check(lib.mc_ray_count(ctx.handle, len(pos), ptr(pos, c_double), ptr(R, c_double), len(dirs),
                                   ptr(dirs, c_double), len(steps), ptr(steps, c_double), STEP, ptr(n, c_int64)))
    hits = np.zeros((len(pos) * len(dirs), 3), np.int32)
    mc._lib.check(lib.mc_ray_hits(ctx.handle, ptr(hits, c_int32)))
    return n, hits.reshape(len(pos), len(dirs), 3), Rinv


def abi_rows(mc, ctx, Rinv, noise, n_hits):
    rows = np.zeros((n_hits, 5), np.float64)
    mc._lib.check(ctx.lib.mc_ray_emit_f64(ctx.handle, ptr(Rinv, c_double), None if noise is None else ptr(noise, c_double),
                                          ptr(rows, c_double)))
    return rows
