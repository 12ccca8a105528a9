"""Helpers of the relative (sensor-frame) SLERP deskew tests (test_relative_cpu.py,
test_gpu_relative.py).  A plain module, deterministic from its seeds; it imports no product code.

Contract (include/mcdeskew.h mc_deskew_relative): with (R_ref, pos_ref) = slerp_pose(table, t_ref),

    p' = R_ref^T ( R(q(t)) p + pos(t) - pos_ref ),   t = t_frame + t_ns * 1e-9.

Here: the float64 oracle from oracle.restatement, its np.longdouble restatement on
rounding.ext_deskew_pose_slerp, numpy emulations of what the device does (the reference pose of
k_pose_at, the fold of csrc/relfold.hpp with its mutants, slerp_core on given records) and of the
two-pass route the fused mode replaces (global deskew into float32, then one inverse matrix per
frame), and the cases.

The bar is rounding.rounded_once_failures(out, oracle, scale, MARGIN * d_ref) with
scale = |p| + |pos(t)| + |pos_ref| and d_ref the oracle's own error against the extended restatement.
"""
import functools

import numpy as np

import rounding as Q
from conftest import scale_of
from oracle import restatement as R

LD = Q.LD
SHIFT = np.array([500000.0, 5400000.0, 300.0])      # a UTM-scale offset of the pose table
KEYFRAME_T = 17.5                                   # a keyframe time outside every frame of every pattern
REFS = ("start", "end", "key")
# (table, pattern) of rounding.slerp_case: the SGPR path with sub-tiles across a segment boundary (and
# the one ~1.45 rad segment), the LDS window, the per-point search, and a frame wider than 64 segments
# whose sub-tile windows take the SGPR path
PAIRS = (("big", "sorted"), ("spike", "sorted"), ("mid", "shuffled"), ("small", "spread"), ("big", "far"))
CASES = [(tb, pt, sh, ref) for tb, pt in PAIRS for sh in (False, True) for ref in REFS]


def _pose(tr, t):
    return R.slerp_pose(tr["time"], tr["position_gps"], tr["orientation_imu"], np.atleast_1d(np.asarray(t, np.float64)))


def reference_times(times, t_ns, ref):
    """Per-frame reference times: the frame's time, the time of its last return (slerp_time(t_frame,
    max t_ns); the frame's time for an empty frame), or KEYFRAME_T."""
    times = np.asarray(times, np.float64)
    if ref == "start":
        return times.copy()
    if ref == "end":
        return np.array([tf + float(np.max(t)) * 1e-9 if len(t) else tf for tf, t in zip(times, t_ns)])
    if ref == "key":
        return np.full(len(times), KEYFRAME_T)
    raise ValueError(ref)


# ----------------------------------------------------------------------------------------------
# the oracle and its extended restatement
# ----------------------------------------------------------------------------------------------
def relative_oracle(xyz, t_ns, t_frame, t_ref, tr):
    """R_ref^T (deskew_pose_slerp(p) - pos_ref) in float64."""
    g = R.deskew_pose_slerp(xyz, t_ns, t_frame, tr)
    Rr, pr = _pose(tr, t_ref)
    return (g - pr[0]) @ Rr[0]


def ext_reference_pose(t_ref, tr):
    """(R_ref, pos_ref) in extended precision: the images of the origin and the three unit vectors at
    t_ns = 0, t_frame = t_ref."""
    img = Q.ext_deskew_pose_slerp(np.vstack([np.zeros(3), np.eye(3)]), np.zeros(4, np.int64), float(t_ref), tr)
    pos = img[0]
    return (img[1:] - pos).T, pos          # column i of R_ref = image(e_i) - pos_ref


def ext_relative(xyz, t_ns, t_frame, t_ref, tr):
    g = Q.ext_deskew_pose_slerp(xyz, t_ns, t_frame, tr)
    Rr, pr = ext_reference_pose(t_ref, tr)
    d = g - pr
    return (d[:, :, None] * Rr[None, :, :]).sum(axis=1)      # R_ref^T d


def relative_scale(xyz, t_ns, t_frame, t_ref, tr):
    _, p = _pose(tr, float(t_frame) + np.asarray(t_ns, np.int64) * 1e-9)
    _, pr = _pose(tr, t_ref)
    return scale_of(xyz, p) + np.linalg.norm(pr[0])


# ----------------------------------------------------------------------------------------------
# numpy emulations of the device formulas (no FMA)
# ----------------------------------------------------------------------------------------------
def emu_pose(sg, time, t):
    """k_pose_at: quaternion (x, y, z, w) and position at time t from the segment records."""
    k = int(np.clip(np.searchsorted(time, t, side="right") - 1, 0, len(time) - 2))
    al = float(np.clip((t - sg["t0"][k]) * sg["inv_dt"][k], 0.0, 1.0))
    cs, sc = Q.cos_sinc(np.array([al * sg["th"][k]]), 10)
    s = al * sc[0]
    return s * sg["v"][k] + cs[0] * sg["q0"][k], al * sg["dp"][k] + sg["p0"][k]


def quat_conj_mul(r, q):
    """relfold.hpp quat_conj_mul: conj(r) (x) q, q (n, 4)."""
    ax, ay, az, aw = -r[0], -r[1], -r[2], r[3]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([aw * x + ax * w + ay * z - az * y,
                     aw * y - ax * z + ay * w + az * x,
                     aw * z + ax * y - ay * x + az * w,
                     aw * w - ax * x - ay * y - az * z], axis=1)


def quat_mul(r, q):
    """r (x) q without the conjugate (the 'conj dropped' mutant)."""
    return quat_conj_mul(np.array([-r[0], -r[1], -r[2], r[3]]), q)


def quat_rot_inv(r, v):
    """relfold.hpp quat_rot_inv: R(r)^T v, v (n, 3)."""
    ux, uy, uz, w = -r[0], -r[1], -r[2], r[3]
    tx = uy * v[:, 2] - uz * v[:, 1]
    ty = uz * v[:, 0] - ux * v[:, 2]
    tz = ux * v[:, 1] - uy * v[:, 0]
    return np.stack([v[:, 0] + 2.0 * (w * tx + (uy * tz - uz * ty)),
                     v[:, 1] + 2.0 * (w * ty + (uz * tx - ux * tz)),
                     v[:, 2] + 2.0 * (w * tz + (ux * ty - uy * tx))], axis=1)


MUTANTS = ("no_conj", "dp_unrotated", "pos_after_rotation")


def fold_records(sg, q_ref, pos_ref, mutant=None):
    """relfold.hpp rel_fold on every record of sg.  Mutants: 'no_conj' (q_ref (x) q instead of
    conj(q_ref) (x) q), 'dp_unrotated' (dp left in the global frame), 'pos_after_rotation'
    (R_ref^T p0 - pos_ref)."""
    assert mutant is None or mutant in MUTANTS
    out = dict(sg)
    qm = quat_mul if mutant == "no_conj" else quat_conj_mul
    out["q0"] = qm(q_ref, sg["q0"])
    out["v"] = qm(q_ref, sg["v"])
    if mutant == "pos_after_rotation":
        out["p0"] = quat_rot_inv(q_ref, sg["p0"]) - pos_ref
    else:
        out["p0"] = quat_rot_inv(q_ref, sg["p0"] - pos_ref)
    out["dp"] = sg["dp"].copy() if mutant == "dp_unrotated" else quat_rot_inv(q_ref, sg["dp"])
    return out


def emu_slerp_records(sg, time, xyz, t_ns, t_frame, K=10):
    """rounding.emu_slerp (slerp_core on float64 numpy) on given segment records instead of
    rounding.pose_segments(tr); with those records it equals emu_slerp bit for bit (test_relative_cpu)."""
    time = np.asarray(time, np.float64)
    tq = float(t_frame) + np.asarray(t_ns, dtype=np.int64) * 1e-9
    k = np.clip(np.searchsorted(time, tq, side="right") - 1, 0, len(time) - 2)
    al = np.clip((tq - sg["t0"][k]) * sg["inv_dt"][k], 0.0, 1.0)
    cs, sc = Q.cos_sinc(al * sg["th"][k], K)
    s = al * sc
    qi = s[:, None] * sg["v"][k] + cs[:, None] * sg["q0"][k]
    qx, qy, qz, qw = qi[:, 0], qi[:, 1], qi[:, 2], qi[:, 3]
    p = np.asarray(xyz, np.float64)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    tx = qy * Z - qz * Y
    ty = qz * X - qx * Z
    tz = qx * Y - qy * X
    cx = qw * tx + (qy * tz - qz * ty)
    cy = qw * ty + (qz * tx - qx * tz)
    cz = qw * tz + (qx * ty - qy * tx)
    c2 = 2.0 * np.stack([cx, cy, cz], axis=1)
    return c2 + ((al[:, None] * sg["dp"][k] + p) + sg["p0"][k])


def emu_folded(xyz, t_ns, t_frame, t_ref, tr, mutant=None, K=10):
    """The batch path: reference pose (k_pose_at), folded records (k_rel_compose), slerp_core; float64
    values before the store's rounding."""
    sg = Q.pose_segments(tr)
    time = np.asarray(tr["time"], np.float64)
    q_ref, pos_ref = emu_pose(sg, time, float(t_ref))
    return emu_slerp_records(fold_records(sg, q_ref, pos_ref, mutant), time, xyz, t_ns, t_frame, K)


def emu_two_pass(xyz, t_ns, t_frame, t_ref, tr, K=10):
    """The route without the fused mode: the global deskew into a float32 batch, then one inverse
    matrix per frame in float64 (mc_transform_affine with [R_ref^T | -R_ref^T pos_ref]); float64
    values before the second store's rounding."""
    g32 = Q.f32(Q.emu_slerp(xyz, t_ns, t_frame, tr, K))
    Rr, pr = _pose(tr, t_ref)
    A = Rr[0].T
    return g32 @ A.T + (-(A @ pr[0]))


# ----------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(table, pattern):
    c = Q.slerp_case(table, pattern)
    return c["tr"], c["times"], c["t_ns"]


def relative_case(table, pattern, shifted, ref, seed=29):
    """rounding.slerp_case's table, frame times and t_ns (COUNTS frames); the pose table's positions as
    generated or shifted by SHIFT; per-frame reference times of kind `ref`; points regenerated with
    rounding.mixed_points for the relative map (M = R_ref^T R(t), t = R_ref^T (pos(t) - pos_ref)), so
    half of them cancel in the reference frame."""
    tr0, times, t_ns = _base(table, pattern)
    tr = dict(tr0)
    if shifted:
        tr["position_gps"] = tr0["position_gps"] + SHIFT
    t_ref = reference_times(times, t_ns, ref)
    rng = Q._rng(seed, Q.SLERP_TABLES.index(table), (Q.PATTERNS + ("far",)).index(pattern), int(shifted), REFS.index(ref))
    xyz = []
    for f, n in enumerate(Q.COUNTS):
        Rm, p = _pose(tr, float(times[f]) + t_ns[f] * 1e-9)
        Rr, pr = _pose(tr, t_ref[f])
        M = np.einsum("ji,njk->nik", Rr[0], Rm)
        tt = (p - pr[0]) @ Rr[0]
        xyz.append(Q.mixed_points(M, tt, rng, n))
    return {"tr": tr, "times": times.copy(), "t_ns": t_ns, "t_ref": t_ref, "xyz": xyz}


def relative_reference(case):
    """Per frame: (oracle64, extended, scale)."""
    out = []
    tr = case["tr"]
    for f, n in enumerate(Q.COUNTS):
        if n == 0:
            out.append((np.zeros((0, 3)), np.zeros((0, 3), LD), np.zeros(0)))
            continue
        a = (case["xyz"][f], case["t_ns"][f], case["times"][f], case["t_ref"][f], tr)
        out.append((relative_oracle(*a), ext_relative(*a), relative_scale(*a)))
    return out


@functools.lru_cache(maxsize=None)
def relative_bundle(table, pattern, shifted, ref):
    """(case, per-frame (oracle64, extended, scale), d_ref): computed once per process, shared by the
    tests, never modified."""
    case = relative_case(table, pattern, shifted, ref)
    frames = relative_reference(case)
    return case, frames, Q.case_d_ref(frames)


def failures(case, frames, d, fn):
    """Coordinates of float32(fn(xyz, t_ns, t_frame, t_ref, tr)) outside the bar, over the frames."""
    bad = 0
    for f, (ref, _, sc) in enumerate(frames):
        if len(ref) == 0:
            continue
        y = fn(case["xyz"][f], case["t_ns"][f], case["times"][f], case["t_ref"][f], case["tr"])
        bad += Q.rounded_once_failures(Q.f32(y), ref, sc, Q.MARGIN * d)
    return bad
