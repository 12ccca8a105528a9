"""Shared fixtures of the scene scanner's edge tests (tests/test_scan_edges_cpu.py,
tests/test_gpu_scan_edges.py): numpy only, deterministic seeds.

scan_environment (LMC:701-770; csrc/scan.hpp) keeps a scene point when d2 <= range_max^2,
sqrt(d2) >= range_min, |atan2(ly, lx)| <= fov_h / 2 and |asin(clip(lz / max(r, 1e-6)))| <= fov_v / 2
(degrees).  ``mask`` restates that decision per point with its signed margins; ``edge_scene`` puts
points on every one of those edges, ulps and 1e-12 .. 1e-2 degrees to either side, under the poses of
``poses_of``; ``cap_scene`` / ``CAP_FRAMES`` put the visible counts on the boundaries of the
systematic subsample.  The 4th column of every scene row is the row's own index, so kept sets are
compared by identity and order.
"""
import numpy as np

from oracle import restatement as R

# (range_min, range_max, fov_horizontal, fov_vertical); half FOVs are fov / 2
CONFIGS = [
    (0.05, 90.0, 70.0, 77.2),      # 0  the defaults
    (0.5, 37.3, 177.9, 1.0),       # 1  half FOVs 88.95 (tan 54.6) and 0.5 degrees
    (0.0, 5.0, 0.0, 177.99),       # 2  range_min 0, half FOVs 0 and 88.995: zero-orientation poses only
    (-1.0, 5.0, 360.0, 180.0),     # 3  fast == 0: everything in range is kept
    (2.0, 50.0, 178.0, 178.0),     # 4  fast == 0: half FOVs of exactly 89
    (2.0, 50.0, 180.0, 90.0),      # 5  fast == 0: half FOV 90
    (2.0, 50.0, -10.0, 90.0),      # 6  fast == 0: negative FOV keeps nothing
    (2.0, 50.0, float("nan"), 90.0),   # 7  fast == 0: NaN FOV keeps nothing
    (0.5, 1.25, 120.0, 80.0),      # 8  dyadic ranges: exact on-edge points exist
    (0.0, 5.0, 70.0, 77.2),        # 9  fast tier with range_min 0: the FOV decides the near-sensor rows over the
                                   #    whole sphere (config 2 keeps only its az = 0 plane): clamp and guard mutants
    (2.0, 50.0, 181.0, 181.0),     # 10 fast == 0 with half FOVs of 90.5: keeps points behind the sensor, which a
                                   #    fast bound above 89 would drop (no config above has a half FOV in (90, 91))
]
DYADIC = 8
FAST = [i for i, c in enumerate(CONFIGS) if 0 <= c[2] / 2 < 89 and 0 <= c[3] / 2 < 89]

POSES = [
    (np.zeros(3), np.zeros(3)),
    (np.array([12.5, -3.25, 1.75]), np.array([0.3, -0.2, 2.5])),
    (np.array([5.8e5, 4.5e6, 30.0]), np.array([-3.0, 1.4, -0.7])),
]
SEED = 20240611
FLOOR_DEG = 1e-12      # GPU floor on the reference's FOV margins (scan section)
NEAR_R = (0.0, 1e-8, 5e-7, 1e-6, 2e-6, 9e-6, 1e-5, 1.1e-5, 1e-4)
ULPS = tuple(range(-6, 7)) + (-1e4, 1e4, -1e7, 1e7)
OFFSETS = np.concatenate([-np.logspace(-12, -2, 60), [0.0], np.logspace(-12, -2, 60)])
CLASSES = ("range_max", "range_min", "az_edge", "el_edge", "corner_az_rmin", "corner_el_rmax", "near",
           "background", "nonfinite", "exact", "pad")


def config_of(cfg, points_per_frame=10 ** 9, noise=0.0) -> dict:
    return {"range_min": cfg[0], "range_max": cfg[1], "fov_horizontal": cfg[2], "fov_vertical": cfg[3],
            "points_per_frame": points_per_frame, "lidar_range_noise": noise}


def poses_of(ci):
    """The poses a config is scanned from: with fov_horizontal == 0 only ly == 0 exactly is inside, which
    a rotated pose cannot place, so that config keeps POSES' translations with zero orientation."""
    if CONFIGS[ci][2] == 0:
        return [(t, np.zeros(3)) for t, _ in POSES]
    return POSES


def mask(env, pos, rpy, cfg):
    """LMC:713-745 per scene point, as oracle.restatement.scan_environment computes it (the same
    prefilter before the matmul, so every product has the oracle's operands and shape).  Returns
    (keep, margins): keep (E,) bool; margins: 'az' = |az| - h and 'el' = |el| - v in degrees (NaN for
    rows the range_max prefilter drops), 'rmin' = sqrt(d2) - range_min, 'rmax' = d2 - range_max^2,
    'az_exact' / 'el_exact': rows whose compared angle is exact under any correctly rounded libm."""
    env = np.asarray(env, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64)
    rmin, rmax, fh, fv = cfg
    E = len(env)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = np.sum((env[:, :3] - pos) ** 2, axis=1)
        pre = d2 <= rmax ** 2
        az = np.full(E, np.nan)
        el = np.full(E, np.nan)
        loc = np.full((E, 3), np.nan)
        s = np.full(E, np.nan)
        if pre.any():
            envf = env[pre]
            Rm = R.euler_xyz_matrix(np.asarray(rpy, dtype=np.float64))
            l = (Rm.T @ (envf[:, :3] - pos).T).T
            rng_ = np.sqrt(d2[pre])
            loc[pre] = l
            s[pre] = np.clip(l[:, 2] / np.maximum(rng_, 1e-6), -1, 1)
            az[pre] = np.arctan2(l[:, 1], l[:, 0]) * 180 / np.pi
            el[pre] = np.arcsin(s[pre]) * 180 / np.pi
        m = {"az": np.abs(az) - fh / 2, "el": np.abs(el) - fv / 2, "rmin": np.sqrt(d2) - rmin,
             "rmax": d2 - rmax ** 2}
        keep = pre & (np.abs(az) <= fh / 2) & (np.abs(el) <= fv / 2) & (np.sqrt(d2) >= rmin)
    # exact by construction.  With zero orientation (R = I on the device and here, loc = p - t exactly):
    # atan2(+-0, x > 0) = +-0, atan2(y, +-0) = +-pi/2 (or +-0), asin(+-0) = +-0.  Under any pose:
    # asin(+-1) = +-pi/2; a sine that clips to +-1 here is compared with a half FOV of 90 (else its
    # margin 90 - v is no small one), which no |asin| exceeds, whatever last bit the device's sine has.
    flat = not np.any(np.asarray(rpy, dtype=np.float64))
    m["az_exact"] = flat & pre & (((loc[:, 1] == 0) & (loc[:, 0] > 0)) | (loc[:, 0] == 0))
    m["el_exact"] = pre & ((flat & (s == 0)) | (np.abs(s) == 1))
    return keep, m


def below_floor(m, floor=FLOOR_DEG):
    """Rows whose decision hangs on an FOV comparison closer than ``floor`` degrees (and not exact by
    construction): in range, no FOV test clearly failed, at least one within the floor."""
    with np.errstate(invalid="ignore"):
        az_unc = (np.abs(m["az"]) < floor) & ~m["az_exact"]
        el_unc = (np.abs(m["el"]) < floor) & ~m["el_exact"]
        in_range = (m["rmax"] <= 0) & (m["rmin"] >= 0)
        return in_range & (az_unc | el_unc) & ((m["az"] <= 0) | az_unc) & ((m["el"] <= 0) | el_unc)


def gpu_asserted(m, floor=FLOOR_DEG):
    """The rows a GPU run is held to: every range decision (d2 and sqrt are exact on both sides, no
    floor), and every FOV decision whose reference margin is at least ``floor`` degrees or whose
    compared angle is exact (mask's az_exact / el_exact)."""
    return ~below_floor(m, floor)


def _sphere(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _local(az_deg, el_deg, r):
    a, e = np.radians(az_deg), np.radians(el_deg)
    return np.column_stack([r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e) * np.ones_like(a)])


def edge_scene(ci, pi, seed=SEED):
    """(env, cls): env (E, 4) world rows [x, y, z, own index] for config ``ci`` seen from
    ``poses_of(ci)[pi]``, shuffled, E > 1024 and no multiple of 1024; cls (E,) index into CLASSES."""
    rmin, rmax, fh, fv = CONFIGS[ci]
    pos, rpy = poses_of(ci)[pi]
    rng = np.random.default_rng([seed, ci, pi])
    h = abs(fh / 2) if np.isfinite(fh) else 35.0      # the angles the points are built around
    v = abs(fv / 2) if np.isfinite(fv) else 35.0
    h_in, v_in = min(h, 180.0), min(v, 90.0)
    lo = max(rmin, 1e-3)
    parts, cls = [], []

    def add(name, loc):
        parts.append(np.asarray(loc, dtype=np.float64).reshape(-1, 3))
        cls.append(np.full(len(parts[-1]), CLASSES.index(name)))

    # range edges: directions well inside the FOV, radii k ulps from range_max / range_min
    daz, dele = rng.uniform(-0.8, 0.8, 400) * h_in, rng.uniform(-0.8, 0.8, 400) * v_in
    unit = _local(daz, dele, 1.0)
    for name, r0 in (("range_max", rmax), ("range_min", lo)):
        for k in ULPS:
            add(name, unit * (r0 + k * np.spacing(r0)))
    # FOV edges: azimuth at a random elevation up to 0.9 v, elevation at a random azimuth up to 0.9 h
    radii = (0.3, 7.7, 0.99 * rmax)
    for r in radii:
        for sgn in (1.0, -1.0):
            n = len(OFFSETS)
            add("az_edge", _local(sgn * (h + OFFSETS), rng.uniform(-0.9, 0.9, n) * v_in, r))
            add("el_edge", _local(rng.uniform(-0.9, 0.9, n) * h_in, sgn * (v + OFFSETS), r))
    # corners: two edges at once
    off = OFFSETS[::4]
    for k in (-3, -1, 0, 1, 3):
        for sgn in (1.0, -1.0):
            n = len(off)
            add("corner_az_rmin", _local(sgn * (h + off), rng.uniform(-0.9, 0.9, n) * v_in, lo + k * np.spacing(lo)))
            add("corner_el_rmax", _local(rng.uniform(-0.9, 0.9, n) * h_in, sgn * (v + off), rmax + k * np.spacing(rmax)))
    # near the sensor: the d2 > 1e-10 guard and the max(r, 1e-6) clamp; 50 directions over the sphere
    # and 12 in the az = 0 half plane (the only ones a fov_horizontal of 0 keeps), |el| up to 89.5
    plane = _local(np.zeros(12), np.array([-89.5, -80, -60, -45, -20, -1, 0, 1, 30, 50, 85, 89.5]), 1.0)
    for r in NEAR_R:
        add("near", np.vstack([_sphere(rng, 50), plane]) * r)
    # background: the whole sphere out to 1.2 range_max, half of it behind the sensor
    bg = _sphere(rng, 3000) * (rng.uniform(0, 1.2, 3000) ** (1 / 3) * rmax)[:, None]
    bg[:, 0] = np.abs(bg[:, 0]) * np.where(np.arange(3000) % 2, 1.0, -1.0)
    add("background", bg)
    # exact on-edge points (zero orientation at the origin only: no rounding between scene and sensor)
    if not np.any(pos) and not np.any(rpy):
        ex = [[rmax, 0, 0], [lo, 0, 0], [np.nextafter(rmax, np.inf), 0, 0], [np.nextafter(lo, 0), 0, 0]]
        if ci == DYADIC:    # dyadic Pythagorean triples: d2 == range_max^2 exactly
            ex += [[0.75, 1.0, 0], [0.75, -1.0, 0], [1.0, 0.75, 0], [1.0, 0, 0.75], [1.0, 0, -0.75], [1.25, 0, -0.0],
                   [0.5, -0.0, 0.0]]
        add("exact", ex)
    loc = np.vstack(parts)
    world = (R.euler_xyz_matrix(rpy) @ loc.T).T + pos if np.any(rpy) else loc + pos
    world = np.vstack([world, [[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf]]])
    cls.append(np.full(3, CLASSES.index("nonfinite")))
    # pad to more than one tile and off the tile size, with rows well inside the FOV
    E = len(world)
    n_pad = (E % 1024 == 0) + max(0, 1100 - E)
    if n_pad:
        padl = _local(rng.uniform(-0.5, 0.5, n_pad) * h_in, rng.uniform(-0.5, 0.5, n_pad) * v_in, 0.5 * (lo + rmax))
        world = np.vstack([world, (R.euler_xyz_matrix(rpy) @ padl.T).T + pos])
        cls.append(np.full(n_pad, CLASSES.index("pad")))
    cls = np.concatenate(cls)
    perm = rng.permutation(len(world))
    env = np.column_stack([world[perm], np.arange(len(world), dtype=np.float64)])
    return env, cls[perm]


def pose_dict(pos, rpy) -> dict:
    return {"position": np.asarray(pos, dtype=np.float64), "orientation": np.asarray(rpy, dtype=np.float64)}


def many_pose_case(ci, seed=SEED):
    """One scene and one trajectory for a launch over several poses: the config's edge scenes of all its
    poses in one scene (ids renumbered), a pose table of those poses and five random ones near the
    second, and 11 frame times (two frame groups) that select table rows by next-or-equal, between
    the table's times and past its end included.  Returns (env, trajectory, frame_times, pose_index)."""
    rng = np.random.default_rng([seed, ci, 99])
    poses = list(poses_of(ci))
    base = poses[1][0]
    for _ in range(5):
        poses.append((base + rng.uniform(-2, 2, 3), rng.uniform(-np.pi, np.pi, 3)))
    env = np.vstack([edge_scene(ci, pi, seed)[0] for pi in range(3)])
    env[:, 3] = np.arange(len(env))
    T = len(poses)
    tr = {"time": np.arange(T, dtype=np.float64) * 0.5,
          "position_gps": np.array([p for p, _ in poses]), "orientation_imu": np.array([o for _, o in poses]),
          "velocity": np.zeros((T, 3))}
    times = np.concatenate([tr["time"], [0.25, 1.75, 99.0]])
    idx = R.select_pose_index(tr["time"], times)
    return env, tr, times, idx


# ---- the subsample's boundaries -------------------------------------------------------------------
CAP = 700
CAP_N = [0, 1, 699, 700, 701, 1399, 1400, 1401, 2099, 2100, 2101, 2200, 2, 350, 1050, 1750, 2199]
CAP_CONFIG = (0.05, 90.0, 70.0, 77.2)
CAPS = (CAP, 1, 10 ** 6)
N_CAP = 2200


def cap_scene():
    """(4400, 4): 2200 points ahead of a sensor looking down +x (x = 1 + 0.01 i, lateral jitter 1e-3),
    each followed by a row no frame sees (behind every pose, or far out of range): visible ranks differ
    from scene indices and the visible points span five scene tiles."""
    rng = np.random.default_rng(SEED + 7)
    i = np.arange(N_CAP)
    vis = np.column_stack([1 + 0.01 * i, rng.uniform(-1e-3, 1e-3, N_CAP), rng.uniform(-1e-3, 1e-3, N_CAP)])
    hid = np.where((i % 2 == 0)[:, None], np.column_stack([-1 - 0.01 * i, 0 * i, 0 * i]),
                   np.column_stack([500.0 + i, 0 * i, 0 * i]))
    env = np.empty((2 * N_CAP, 4))
    env[0::2, :3] = vis
    env[1::2, :3] = hid
    env[:, 3] = np.arange(2 * N_CAP)
    return env


def cap_frames():
    """CAP_FRAMES: 17 zero-orientation poses on the x axis (three frame groups, the last partial); pose f
    sees exactly the last CAP_N[f] of the 2200 points (the others are nearer than range_min or behind)."""
    x = [100.0 if n == 0 else 1 + 0.01 * (N_CAP - n) - 0.055 for n in CAP_N]
    F = len(x)
    return {"time": np.arange(F, dtype=np.float64), "position_gps": np.column_stack([x, np.zeros(F), np.zeros(F)]),
            "orientation_imu": np.zeros((F, 3)), "velocity": np.zeros((F, 3))}


CAP_FRAMES = cap_frames()


def subsample(ids, cap):
    """LMC:757-762 on the visible ids: every (n // cap)-th, at most cap."""
    n = len(ids)
    return ids[np.arange(0, n, n // cap)[:cap]] if n > cap else ids


def subsample_count(n, cap):
    return min(cap, -(-n // (n // cap))) if n > cap else n
