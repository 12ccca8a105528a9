"""The "float64, rounded once" bar for the float32 batch kernels (test_rounding_cpu.py,
test_gpu_rounding.py).  A plain module, deterministic from its seeds; it imports no product code.

DESIGN §3/§4 and csrc/kernels.hpp promise that every batch kernel forms each output coordinate in
float64 and rounds it once to float32.  conftest.assert_scaled_close (1e-5 relative) is ten orders of
magnitude above that arithmetic; ``rounded_once_failures`` is the sharp bar beside it:

  an output coordinate y passes when  float32(ref - delta * scale) <= y <= float32(ref + delta * scale),

i.e. when some float64 value within delta * scale of the oracle rounds to y (scale = |p| + |t| per
point, conftest.scale_of).  On an ordinary coordinate that is bitwise equality with float32(oracle)
except within delta * scale of a rounding boundary; on a coordinate that cancels to ~1e-7 * scale the
float32 ulp is ~1e-14 * scale and the bar is an absolute float64-level check (``cancelling_points``
builds such inputs).

delta = MARGIN * d_ref(case): d_ref is the oracle's own float64 error, max |oracle - extended| / scale
against the np.longdouble restatements below (``ext_*``; they start from the float64 inputs as the
reference forms them and run everything after in extended precision).  MARGIN multiplies a quantity
measured against the reference, never the kernels' output.

Besides: numpy float64 emulations of slerp_core / imu_core / sincos_prep (test-side restatements of the
formulas in kernels.hpp) with a selectable polynomial length and the defects the bar has to see, and
the inputs of the GPU cases (so their d_ref is computed, and bounded, without a GPU).
"""
import functools
import math
from fractions import Fraction

import numpy as np

from conftest import scale_of
from oracle import restatement as R

LD = np.longdouble
# delta = MARGIN * d_ref.  16: the device evaluates another float64 formula than the oracle
# (reciprocal multiply, FMA, a 2.4-ulp sin / cos, a few dozen roundings); at 16 * d_ref the correct
# emulations pass and every mutation of test_rounding_cpu.py fails.
MARGIN = 16.0
D_REF_MAX = 1e-13          # an ill-conditioned case would make the bar vacuous

SUB = 1024                 # points of a sub-tile (kernels.hpp kBlock float4 groups)
COUNTS = (4096, 1025, 257, 1, 0, 3000)
PATTERNS = ("sorted", "shuffled", "spread")


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def f32(a):
    """float64 array of float32 values (what a float32 batch column holds exactly)."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------------------------
# the bar
# ----------------------------------------------------------------------------------------------
def rounded_once_failures(y32, ref64, scale, delta):
    """Output coordinates outside [float32(ref - delta * scale), float32(ref + delta * scale)]
    (numpy round-to-nearest casts; NaN counts as outside).  y32 (n, 3) float32 values (any float
    dtype holding them), ref64 (n, 3), scale (n,)."""
    y = np.asarray(y32)
    assert np.array_equal(y.astype(np.float32).astype(y.dtype), y, equal_nan=True), "y32 must hold float32 values"
    y = y.astype(np.float32)
    ref = np.asarray(ref64, dtype=np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    w = float(delta) * np.asarray(scale, dtype=np.float64)
    if ref.ndim == 2:
        w = w[:, None]
    with np.errstate(over="ignore"):
        lo = (ref - w).astype(np.float32)
        hi = (ref + w).astype(np.float32)
    return int(np.count_nonzero(~((y >= lo) & (y <= hi))))


def d_ref(oracle64, extended, scale):
    """max |oracle64 - extended| / scale over the points (0.0 for an empty case)."""
    o = np.asarray(oracle64, dtype=np.float64)
    if o.size == 0:
        return 0.0
    e = np.abs(o.astype(LD) - np.asarray(extended, dtype=LD))
    if e.ndim == 2:
        e = e.max(axis=1)
    return float((e / np.maximum(np.asarray(scale, dtype=LD), LD(1e-30))).max())


def worst_scaled(out, ref, scale):
    out = np.asarray(out, dtype=np.float64)
    if out.size == 0:
        return 0.0
    return float((np.abs(out - np.asarray(ref, np.float64)).max(axis=1) / np.maximum(scale, 1e-30)).max())


# ----------------------------------------------------------------------------------------------
# extended-precision restatements
# ----------------------------------------------------------------------------------------------
def ext_euler_matrix(rpy):
    """R = Rz(yaw) Ry(pitch) Rx(roll) of float64 (or already extended) angles."""
    rpy = np.asarray(rpy).astype(LD)
    r, p, y = rpy[..., 0], rpy[..., 1], rpy[..., 2]
    sr, cr, sp, cp, sy, cy = np.sin(r), np.cos(r), np.sin(p), np.cos(p), np.sin(y), np.cos(y)
    M = np.empty(rpy.shape[:-1] + (3, 3), dtype=LD)
    M[..., 0, 0] = cy * cp
    M[..., 0, 1] = cy * sp * sr - sy * cr
    M[..., 0, 2] = cy * sp * cr + sy * sr
    M[..., 1, 0] = sy * cp
    M[..., 1, 1] = sy * sp * sr + cy * cr
    M[..., 1, 2] = sy * sp * cr - cy * sr
    M[..., 2, 0] = -sp
    M[..., 2, 1] = cp * sr
    M[..., 2, 2] = cp * cr
    return M


def ext_euler_quat(rpy):
    h = np.asarray(rpy, dtype=np.float64).astype(LD) * LD(0.5)
    sr, cr = np.sin(h[..., 0]), np.cos(h[..., 0])
    sp, cp = np.sin(h[..., 1]), np.cos(h[..., 1])
    sy, cy = np.sin(h[..., 2]), np.cos(h[..., 2])
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def _matvec(M, v):
    return (M * v[..., None, :]).sum(axis=-1)


def ext_transform_pointcloud(xyz, rotation, translation):
    """LMC:772-776, R(rpy) p + t."""
    return _matvec(ext_euler_matrix(rotation), np.asarray(xyz, np.float64).astype(LD)) \
        + np.asarray(translation, np.float64).astype(LD)


def ext_affine(xyz, M, w=None):
    """CSIM:214-233, A p + b w with [A | b] = M[:3, :4] (w = 1 without a homogeneous column)."""
    M = np.asarray(M, np.float64).astype(LD)
    p = np.asarray(xyz, np.float64).astype(LD)
    ww = LD(1.0) if w is None else np.asarray(w, np.float64).astype(LD)[:, None]
    return _matvec(M[:3, :3], p) + M[:3, 3] * ww


def ext_deskew_pose_slerp(xyz, t_ns, t_frame, tr):
    """oracle.deskew_pose_slerp from tq = t_frame + t_ns * 1e-9 (float64, as the reference forms it)
    on: Theta = 2 atan2(|q1 - q0|, |q1 + q0|), every later step in extended precision."""
    time = np.asarray(tr["time"], np.float64)
    tq = float(t_frame) + np.asarray(t_ns, dtype=np.int64) * 1e-9
    T = len(time)
    q = ext_euler_quat(tr["orientation_imu"])
    pos = np.asarray(tr["position_gps"], np.float64).astype(LD)
    p = np.asarray(xyz, np.float64).astype(LD)
    assert T >= 2
    k = np.clip(np.searchsorted(time, tq, side="right") - 1, 0, T - 2)
    dt = time[k + 1].astype(LD) - time[k].astype(LD)
    al = np.where(dt > 0, (tq.astype(LD) - time[k].astype(LD)) / np.where(dt > 0, dt, LD(1)), LD(0))
    al = np.clip(al, LD(0), LD(1))
    q0, q1 = q[k], q[k + 1].copy()
    neg = (q0 * q1).sum(axis=1) < 0
    q1[neg] = -q1[neg]
    th = 2 * np.arctan2(np.sqrt(((q1 - q0) ** 2).sum(axis=1)), np.sqrt(((q1 + q0) ** 2).sum(axis=1)))
    zero = th == 0
    sn = np.where(zero, LD(1), np.sin(th))
    s1 = np.where(zero, al, np.sin(al * th) / sn)
    s0 = np.where(zero, 1 - al, np.sin((1 - al) * th) / sn)
    qi = s0[:, None] * q0 + s1[:, None] * q1
    qi = qi / np.sqrt((qi ** 2).sum(axis=1))[:, None]
    x, y, z, w = qi[:, 0], qi[:, 1], qi[:, 2], qi[:, 3]
    M = np.empty((len(qi), 3, 3), dtype=LD)
    M[:, 0, 0] = 1 - 2 * (y * y + z * z)
    M[:, 0, 1] = 2 * (x * y - z * w)
    M[:, 0, 2] = 2 * (x * z + y * w)
    M[:, 1, 0] = 2 * (x * y + z * w)
    M[:, 1, 1] = 1 - 2 * (x * x + z * z)
    M[:, 1, 2] = 2 * (y * z - x * w)
    M[:, 2, 0] = 2 * (x * z - y * w)
    M[:, 2, 1] = 2 * (y * z + x * w)
    M[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return _matvec(M, p) + pos[k] + al[:, None] * (pos[k + 1] - pos[k])


def ext_compensate_arrays(xyz, t_abs, start, imu_ts, gyro):
    """oracle.compensate_arrays from dt = (t - start) * 1e-9 (float64) and the float64 gyro table on."""
    imu_ts = np.asarray(imu_ts, np.int64)
    g = np.asarray(gyro, np.float64).astype(LD)
    t = np.asarray(t_abs, np.int64)
    M = len(imu_ts)
    c = np.searchsorted(imu_ts, t, side="right")
    b = np.clip(c - 1, 0, M - 1)
    a = np.clip(c, 0, M - 1)
    den = (imu_ts[a] - imu_ts[b]).astype(LD)
    al = np.where((c > 0) & (c < M), (t - imu_ts[b]).astype(LD) / np.where(den > 0, den, LD(1)), LD(0))
    w = g[b] + al[:, None] * (g[a] - g[b])
    dt = ((t - int(start)) * 1e-9).astype(LD)
    Rm = ext_euler_matrix(w * dt[:, None])
    return (Rm * np.asarray(xyz, np.float64).astype(LD)[:, :, None]).sum(axis=1)     # R^T p


def ext_scan_local(env_xyz, position, orientation, noise):
    """LMC:726-728, 768: R^T (p - t) + noise of the kept scene points."""
    d = np.asarray(env_xyz, np.float64).astype(LD) - np.asarray(position, np.float64).astype(LD)
    Rm = ext_euler_matrix(orientation)
    return (Rm[None, :, :] * d[:, :, None]).sum(axis=1) + np.asarray(noise, np.float64).astype(LD)


# ----------------------------------------------------------------------------------------------
# inputs that cancel
# ----------------------------------------------------------------------------------------------
def cancelling_points(M, t, rng, n=None):
    """Points p = float32(M^-1 (c - t)) whose image c = M p + t cancels: for half of the points every
    component of c is 1e-7 .. 1e-3 of the point's scale |p| + |t| (only where |t| >= 1: without a
    translation |c| = |p|), for the others one component is.  M (3, 3) or (n, 3, 3): the matrix the
    operation applies to the point; t (3,) or (n, 3).  Returns (n, 3) float64 holding float32 values."""
    M = np.asarray(M, np.float64)
    t = np.asarray(t, np.float64)
    if n is None:
        n = len(M) if M.ndim == 3 else len(t)
    M = np.broadcast_to(M, (n, 3, 3))
    t = np.broadcast_to(t, (n, 3))
    tn = np.linalg.norm(t, axis=1)
    small = 10.0 ** rng.uniform(-7.0, -3.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    c = rng.uniform(-90.0, 90.0, (n, 3))
    j = rng.integers(0, 3, n)
    rows = np.arange(n)
    c[rows, j] = 0.0
    sc = np.linalg.norm(c - t, axis=1) + tn                        # ~ |p| + |t| of the single-component half
    c[rows, j] = small[rows, j] * sc
    every = ((rows // 2) % 2 == 0) & (tn >= 1.0)
    c[every] = small[every] * (2.0 * tn[every])[:, None]           # |p| ~ |t|
    return f32(np.linalg.solve(M, (c - t)[:, :, None])[:, :, 0])


def mixed_points(M, t, rng, n):
    """n float32-valued points: the even half random in +-90 m, the odd half cancelling_points of the
    per-point (M, t) (shuffled together by position, deterministically)."""
    p = f32(rng.uniform(-90.0, 90.0, (n, 3)))
    if n:
        c = cancelling_points(M, t, rng, n)
        odd = np.arange(n) % 2 == 1
        p[odd] = c[odd]
    return p


# ----------------------------------------------------------------------------------------------
# float64 emulations of the device formulas (kernels.hpp), no FMA
# ----------------------------------------------------------------------------------------------
def poly_coeffs(K):
    """(cos, sinc) Taylor coefficients after the leading 1: c[k] of z^(k+1), as kPoly4/6/10."""
    c = [(-1.0) ** (k + 1) / float(math.factorial(2 * k + 2)) for k in range(K)]
    s = [(-1.0) ** (k + 1) / float(math.factorial(2 * k + 3)) for k in range(K)]
    return np.array(c), np.array(s)


def _horner1(c, z):
    p = np.full_like(z, c[-1])
    for k in range(len(c) - 2, -1, -1):
        p = z * p + c[k]
    return z * p + 1.0


def cos_sinc(x, K, coeffs=None):
    """cos(x), sin(x)/x: K in {4, 6, 10} polynomial terms in z = x^2, or K = 'libm'."""
    if K == "libm":
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.cos(x), np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x))
    c, s = coeffs if coeffs is not None else poly_coeffs(K)
    z = x * x
    return _horner1(c, z), _horner1(s, z)


def quat_of(rpy):
    return R.euler_xyz_quat(rpy)


def pose_segments(tr):
    """PoseSeg of every segment (kernels.hpp pose_seg_q): q0, v = Theta (q1 - cos Theta q0) / sin Theta,
    p0, dp, Theta, t0, 1 / dt."""
    time = np.asarray(tr["time"], np.float64)
    q = quat_of(np.asarray(tr["orientation_imu"], np.float64))
    pos = np.asarray(tr["position_gps"], np.float64)
    q0, q1 = q[:-1], q[1:].copy()
    neg = (q0 * q1).sum(axis=1) < 0
    q1[neg] = -q1[neg]
    th = 2.0 * np.arctan2(np.sqrt(((q1 - q0) ** 2).sum(axis=1)), np.sqrt(((q1 + q0) ** 2).sum(axis=1)))
    ratio = np.where(th > 0, th / np.where(th > 0, np.sin(th), 1.0), 1.0)
    v = ratio[:, None] * (q1 - np.cos(th)[:, None] * q0)
    dt = time[1:] - time[:-1]
    inv_dt = np.where(dt > 0, 1.0 / np.where(dt > 0, dt, 1.0), 0.0)
    return dict(q0=q0, v=v, p0=pos[:-1], dp=pos[1:] - pos[:-1], th=th, t0=time[:-1], inv_dt=inv_dt)


def emu_slerp(xyz, t_ns, t_frame, tr, K, alpha32=False, rot32=False, coeffs=None, fused_time=False):
    """slerp_core on float64 numpy; defects: alpha32 (alpha through float32), rot32 (the rotated point
    rounded to float32 before the translation is added), coeffs (another coefficient set), fused_time
    (t_frame + t_ns * 1e-9 rounded once, as a fused multiply-add forms it, not product then sum)."""
    sg = pose_segments(tr)
    time = np.asarray(tr["time"], np.float64)
    tq = float(t_frame) + np.asarray(t_ns, dtype=np.int64) * 1e-9
    if fused_time:
        tq = (LD(float(t_frame)) + np.asarray(t_ns, dtype=np.int64).astype(LD) * LD(1e-9)).astype(np.float64)
    k = np.clip(np.searchsorted(time, tq, side="right") - 1, 0, len(time) - 2)
    al = np.clip((tq - sg["t0"][k]) * sg["inv_dt"][k], 0.0, 1.0)
    if alpha32:
        al = f32(al)
    cs, sc = cos_sinc(al * sg["th"][k], K, coeffs)
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
    tl = al[:, None] * sg["dp"][k] + sg["p0"][k]
    if rot32:
        return f32(p + c2) + tl
    return c2 + ((al[:, None] * sg["dp"][k] + p) + sg["p0"][k])


def emu_imu(xyz, t_abs, start, imu_ts, gyro, K, alpha32=False, coeffs=None):
    """imu_core on float64 numpy (K = 'libm': the general tier, libm standing in for sincos_prep)."""
    ts = np.asarray(imu_ts, np.int64)
    g = np.asarray(gyro, np.float64)
    t = np.asarray(t_abs, np.int64)
    M = len(ts)
    k = np.clip(np.searchsorted(ts, t, side="right") - 1, 0, M - 1)
    k1 = np.clip(k + 1, 0, M - 1)
    dtn = (ts[k1] - ts[k]).astype(np.float64)
    inv_dt = np.where(dtn > 0, 1.0 / np.where(dtn > 0, dtn, 1.0), 0.0)
    dg = g[k1] - g[k]
    al = np.maximum((t - ts[k]).astype(np.float64) * inv_dt, 0.0)
    if alpha32:
        al = f32(al)
    dt = (t - int(start)).astype(np.float64) * 1e-9
    th = (al[:, None] * dg + g[k]) * dt[:, None]
    cs, sc = cos_sinc(th, K, coeffs)
    sn = th * sc
    sa, sb, s_c = sn[:, 0], sn[:, 1], sn[:, 2]
    ca, cb, cc = cs[:, 0], cs[:, 1], cs[:, 2]
    p = np.asarray(xyz, np.float64)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    x1 = cc * X + s_c * Y
    y1 = -s_c * X + cc * Y
    x2 = cb * x1 - sb * Z
    z2 = sb * x1 + cb * Z
    y3 = ca * y1 + sa * z2
    z3 = -sa * y1 + ca * z2
    return np.stack([x2, y3, z3], axis=1)


# ---- sincos_prep (scalar, exact fma) ---------------------------------------------------------
try:
    _fma = math.fma
except AttributeError:
    def _fma(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c))     # one rounding, to nearest even

PIO2 = (1.57079632673412561417e+00, 6.07710050630396597660e-11, 2.02226624871116645580e-21)   # fdlibm pio2_1/2/3
_S = (1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06,
      -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01)
_C = (-1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07,
      2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02)


def sincos_prep(x, parts=(0, 1, 2)):
    """kernels.hpp sincos_prep: Cody-Waite reduction by pi/2 in the fdlibm parts ``parts`` (all three: the kernel),
    then the fdlibm __kernel_sin / __kernel_cos polynomials.  Returns (sin, cos)."""
    x = float(x)
    n = float(np.rint(x * 6.36619772367581382433e-01))
    r = x
    for k in parts:
        r = _fma(-n, PIO2[k], r)
    z = r * r
    ps = _fma(z, _S[0], _S[1])
    for c in _S[2:]:
        ps = _fma(z, ps, c)
    sr = _fma(r * z, ps, r)
    pc = _fma(z, _C[0], _C[1])
    for c in _C[2:]:
        pc = _fma(z, pc, c)
    hz = 0.5 * z
    w = 1.0 - hz
    cr = w + (((1.0 - w) - hz) + z * z * pc)
    q = int(n)
    s0, c0 = (cr, sr) if q & 1 else (sr, cr)
    return (-s0 if q & 2 else s0), (-c0 if (q + 1) & 2 else c0)


# ----------------------------------------------------------------------------------------------
# the GPU cases' inputs (built on the CPU; test_rounding_cpu.py bounds their d_ref)
# ----------------------------------------------------------------------------------------------
def frame_t_ns(pattern, n, rng, window_ns=6_000_000, last_ns=94_000_000, step_ns=32_000_000):
    """int64 frame-relative times of an n-point frame.
    sorted:   non-decreasing; every 1024-point sub-tile spans ``window_ns`` (at most two 10 ms pose or
              5 ms IMU segments: the SGPR path, most sub-tiles across a segment boundary), the last one
              starting at ``last_ns``, earlier ones ``step_ns`` apart before it;
    shuffled: unsorted over [0, 100 ms) (10 pose / 20 IMU segments: the LDS window);
    spread:   unsorted over +-1.5 s (more than 64 segments in a sub-tile: the per-point search)."""
    if pattern == "sorted":
        nsub = max(1, -(-n // SUB))
        sub = np.arange(n) // SUB
        off = last_ns - step_ns * (nsub - 1 - sub)
        t = off + rng.integers(0, window_ns, n)
        for s in range(nsub):
            m = sub == s
            t[m] = np.sort(t[m])
        return t.astype(np.int64)
    if pattern == "shuffled":
        return rng.integers(0, 100_000_000, n).astype(np.int64)
    if pattern == "spread":
        return rng.integers(-1_500_000_000, 1_500_000_000, n).astype(np.int64)
    raise ValueError(pattern)


# ---- SLERP ----
POSE_T = 4097                                   # 100 Hz rows
THETA_RANGE = {"small": (0.0, 1.0 / 16), "mid": (1.0 / 16, 0.25), "big": (0.25, 1.45)}
_YAW_STEP = {"small": (0.01, 0.10), "mid": (0.16, 0.46), "big": (0.56, 2.86)}
SPIKE_ROW = 1234                                # "spike": segment [1234, 1235] alone has Theta ~ 1.45
SLERP_TABLES = ("small", "mid", "big", "spike")
SLERP_FRAME_TIMES = np.array([12.3081, 3.0042, 25.5513, 33.0004, 8.0, 38.2055])   # "spike": frames 0, 1 meet row 1234


def pose_table(kind, seed=7):
    """100 Hz pose table of POSE_T rows whose segment angles Theta (half the rotation between
    neighbours) lie in THETA_RANGE[kind]; "spike": THETA_RANGE["small"] but for one segment of ~1.45."""
    rng = _rng(seed, SLERP_TABLES.index(kind))
    T = POSE_T
    lo, hi = _YAW_STEP["small" if kind == "spike" else kind]
    step = rng.uniform(lo, hi, T) * rng.choice([-1.0, 1.0], T)
    if kind == "spike":
        step[SPIKE_ROW + 1] = 2.88
    yaw = (np.cumsum(step) + np.pi) % (2.0 * np.pi) - np.pi
    rpy = np.column_stack([rng.normal(0.0, 0.004, T), rng.normal(0.0, 0.004, T), yaw])
    pos = np.array([100.0, -200.0, 5.0]) + np.cumsum(rng.normal(0.0, 0.3, (T, 3)), axis=0)
    return {"time": np.arange(T) * 0.01, "position_gps": pos, "orientation_imu": rpy}


def segment_thetas(tr):
    return pose_segments(tr)["th"]


def slerp_case(table, pattern, seed=11):
    """One batch: COUNTS frames of one time pattern over one table.  "far" (pattern): frame 0's
    sub-tiles are 6 ms windows 0.4 s apart, so the frame spans > 64 segments, its sub-tile windows
    still take the SGPR path, and the first and last lie outside k_prep's 64-sample probe window."""
    tr = pose_table(table)
    rng = _rng(seed, SLERP_TABLES.index(table), (PATTERNS + ("far",)).index(pattern))
    times = SLERP_FRAME_TIMES.copy()
    if table == "spike" and pattern == "sorted":
        # frame 0: its last sub-tile [94, 100) ms over row 1234's start at 12.34 s; frame 1 (two
        # sub-tiles, the second one point) the same
        times[0] = 12.34 - 0.097
        times[1] = 12.34 - 0.0945
    t_ns, xyz = [], []
    for f, n in enumerate(COUNTS):
        if pattern == "far":
            t = frame_t_ns("sorted", n, rng, step_ns=400_000_000, last_ns=1_294_000_000 if f == 0 else 94_000_000)
        else:
            t = frame_t_ns(pattern, n, rng)
        Rm, p = R.slerp_pose(tr["time"], tr["position_gps"], tr["orientation_imu"], float(times[f]) + t * 1e-9)
        t_ns.append(t)
        xyz.append(mixed_points(Rm, p, rng, n))
    return {"tr": tr, "times": times, "t_ns": t_ns, "xyz": xyz}


SLERP_CASES = [(tb, pt) for tb in SLERP_TABLES for pt in PATTERNS] + [("big", "far")]


def slerp_reference(case):
    """Per frame: (oracle64, extended, scale)."""
    out = []
    tr = case["tr"]
    for f, n in enumerate(COUNTS):
        xyz, t = case["xyz"][f], case["t_ns"][f]
        if n == 0:
            out.append((np.zeros((0, 3)), np.zeros((0, 3), LD), np.zeros(0)))
            continue
        ref = R.deskew_pose_slerp(xyz, t, case["times"][f], tr)
        _, p = R.slerp_pose(tr["time"], tr["position_gps"], tr["orientation_imu"], float(case["times"][f]) + t * 1e-9)
        out.append((ref, ext_deskew_pose_slerp(xyz, t, case["times"][f], tr), scale_of(xyz, p)))
    return out


# ---- IMU ----
IMU_HZ_NS = 5_000_000                            # 200 Hz
IMU_ROWS = 801
IMU_THETA = (0.062, 0.063, 0.249, 0.251, 0.8, 30.0)     # max |theta| of a case's points
IMU_STARTS = 1_500_000_000 + np.arange(len(COUNTS), dtype=np.int64) * 200_000_000 + 1_234_567
IMU_FLIP_ROW = 320                               # the rate flips sign from this sample on (ts = 1.6 s:
                                                 # inside frame 0's last "sorted" sub-tile)
_T_MAX = {"sorted": 0.1, "shuffled": 0.1, "spread": 1.5}
IMU_CASES = [(th, pt) for th in IMU_THETA for pt in PATTERNS]


def imu_table(theta_max, pattern, seed=5):
    """200 Hz gyro table: rate (1, -0.6, 0.9) * r * (1 - 0.002 u_k), u_k in [0, 1), r = theta_max over
    the pattern's largest |t|, sign flipped from sample IMU_FLIP_ROW on."""
    rng = _rng(seed, int(theta_max * 1000))
    ts = np.arange(IMU_ROWS, dtype=np.int64) * IMU_HZ_NS
    r = theta_max / _T_MAX[pattern]
    gyro = r * np.array([1.0, -0.6, 0.9]) * (1.0 - 0.002 * rng.random((IMU_ROWS, 1)))
    gyro[IMU_FLIP_ROW:] *= -1.0
    return ts, gyro


def imu_rotation(t_abs, start, ts, gyro):
    """the matrix compensate_arrays applies to each point, R(theta)^T"""
    w = R.imu_interpolate_gyro(ts, gyro, t_abs)
    dt = (np.asarray(t_abs, np.int64) - int(start)) * 1e-9
    return np.swapaxes(R.euler_xyz_matrix(w * dt[:, None]), 1, 2)


def imu_case(theta_max, pattern, seed=13):
    ts, gyro = imu_table(theta_max, pattern)
    rng = _rng(seed, int(theta_max * 1000), PATTERNS.index(pattern))
    t_ns, xyz = [], []
    for f, n in enumerate(COUNTS):
        t = frame_t_ns(pattern, n, rng)
        if pattern == "sorted" and f == 0:
            t[0] = -2_000_000                    # a point before the frame start
        t_ns.append(t)
        xyz.append(mixed_points(imu_rotation(IMU_STARTS[f] + t, IMU_STARTS[f], ts, gyro), np.zeros(3), rng, n))
    return {"ts": ts, "gyro": gyro, "starts": IMU_STARTS.copy(), "t_ns": t_ns, "xyz": xyz}


def imu_reference(case):
    out = []
    for f, n in enumerate(COUNTS):
        xyz, t_abs = case["xyz"][f], case["starts"][f] + case["t_ns"][f]
        if n == 0:
            out.append((np.zeros((0, 3)), np.zeros((0, 3), LD), np.zeros(0)))
            continue
        out.append((R.compensate_arrays(xyz, t_abs, case["starts"][f], case["ts"], case["gyro"]),
                    ext_compensate_arrays(xyz, t_abs, case["starts"][f], case["ts"], case["gyro"]), scale_of(xyz)))
    return out


# ---- frame mode ----
FRAME_COUNTS = (2049, 256, 255, 1, 0)
FRAME_CASES = ("order1", "order1e3", "order1e6", "searchsorted")


def frame_poses(order, seed=3):
    """5 poses: Euler angles of the given order of magnitude, two of every pose's three angles at a
    multiple of pi/2 +- 1e-9; translations at highway scale (5e5 m)."""
    rng = _rng(seed, int(order))
    rpy = rng.uniform(-1.0, 1.0, (5, 3)) * order
    for k in range(5):
        m = np.rint(rng.uniform(-1.0, 1.0, 2) * order / (np.pi / 2))
        rpy[k, [k % 3, (k + 1) % 3]] = m * (np.pi / 2) + np.array([1e-9, -1e-9])
    pos = rng.uniform(-1.0, 1.0, (5, 3)) * 5e5
    return pos, rpy


def frame_case(name, seed=17):
    """pose_select 'direct' with 5 poses of one magnitude, or 'searchsorted' over the 15 poses of all
    three (frame times between, on, before and after the table's entries)."""
    rng = _rng(seed, FRAME_CASES.index(name))
    if name == "searchsorted":
        pp = [frame_poses(o) for o in (1.0, 1e3, 1e6)]
        pos, rpy = np.vstack([p[0] for p in pp]), np.vstack([p[1] for p in pp])
        time = 10.0 + 0.1 * np.arange(15)
        ftimes = np.array([10.05, time[7], 9.0, 99.0, 11.31])
        idx = R.select_pose_index(time, ftimes)
        select = "searchsorted"
    else:
        pos, rpy = frame_poses({"order1": 1.0, "order1e3": 1e3, "order1e6": 1e6}[name])
        time, ftimes, idx, select = np.arange(5.0), np.arange(5.0), np.arange(5), "direct"
    xyz = [mixed_points(R.euler_xyz_matrix(rpy[k]), pos[k], rng, n) for n, k in zip(FRAME_COUNTS, idx)]
    return {"time": time, "pos": pos, "rpy": rpy, "ftimes": ftimes, "idx": idx, "select": select, "xyz": xyz}


def frame_reference(case):
    out = []
    for f, n in enumerate(FRAME_COUNTS):
        k = case["idx"][f]
        xyz = case["xyz"][f]
        ref = R.transform_pointcloud(np.column_stack([xyz, np.zeros(n)]),
                                     {"translation": case["pos"][k], "rotation": case["rpy"][k]})[:, :3]
        out.append((ref, ext_transform_pointcloud(xyz, case["rpy"][k], case["pos"][k]), scale_of(xyz, case["pos"][k])))
    return out


# ---- affine ----
AFFINE_CASES = [(w, m) for w in (False, True) for m in ("one", "per_frame")]
UTM_T = np.array([5.0e5, 4.5e6, 120.0])


def affine_case(w_column, mats, seed=19):
    rng = _rng(seed, int(w_column), ("one", "per_frame").index(mats))
    nm = 1 if mats == "one" else len(FRAME_COUNTS)
    M = np.zeros((nm, 4, 4))
    M[:, 3, 3] = 1.0
    for k in range(nm):
        A = R.euler_xyz_matrix(rng.uniform(-np.pi, np.pi, 3)) @ np.diag(rng.uniform(0.5, 2.0, 3))
        M[k, :3, :3] = A + rng.normal(0.0, 0.05, (3, 3))
        M[k, :3, 3] = UTM_T if k == 0 else rng.normal(0.0, 300.0, 3)
    xyz, w = [], []
    for f, n in enumerate(FRAME_COUNTS):
        m = M[0 if nm == 1 else f]
        wf = f32(rng.uniform(0.5, 1.5, n)) if w_column else np.ones(n)
        # p' = A p + b w: the cancelling half against the translation b w of its own point
        xyz.append(mixed_points(m[:3, :3], m[:3, 3][None, :] * wf[:, None], rng, n))
        w.append(wf if w_column else f32(rng.uniform(0.0, 1.0, n)))      # else: an intensity column, passed through
    return {"M": M, "xyz": xyz, "w": w, "w_column": w_column}


def affine_reference(case):
    out = []
    nm = len(case["M"])
    for f, n in enumerate(FRAME_COUNTS):
        m = case["M"][0 if nm == 1 else f]
        xyz, w = case["xyz"][f], case["w"][f]
        rows = np.column_stack([xyz, w]) if case["w_column"] else xyz
        ref = R.transform_points_h(rows, m) if n else np.zeros((0, 3))
        tw = m[:3, 3][None, :] * (w[:, None] if case["w_column"] else np.ones((n, 1)))
        out.append((ref, ext_affine(xyz, m, w if case["w_column"] else None), scale_of(xyz, tw)))
    return out


# ---- scan ----
SCAN_CFG = dict(range_max=90.0, range_min=0.5, fov_horizontal=70.4, fov_vertical=77.2,
                points_per_frame=300, lidar_range_noise=0.02)
SCAN_SEED = 77


def scan_case(seed=23):
    """A 5000-point scene around 4 poses (direct selection)."""
    rng = _rng(seed)
    pos = np.array([300.0, -120.0, 2.0]) + rng.normal(0.0, 3.0, (4, 3))
    rpy = np.column_stack([rng.normal(0, 0.05, 4), rng.normal(0, 0.05, 4), rng.uniform(-np.pi, np.pi, 4)])
    env = np.column_stack([pos[0, 0] + rng.uniform(-100, 100, 5000), pos[0, 1] + rng.uniform(-100, 100, 5000),
                           rng.uniform(-10, 25, 5000), f32(rng.uniform(0, 1, 5000))])
    return {"env": env, "pos": pos, "rpy": rpy}


def scan_kept(env, position, orientation, config):
    """Indices into env of the points oracle.scan_environment keeps, in its order (LMC:709-762)."""
    env = np.asarray(env, np.float64)
    pos = np.asarray(position, np.float64)
    d2 = np.sum((env[:, :3] - pos) ** 2, axis=1)
    keep = np.flatnonzero(d2 <= config["range_max"] ** 2)
    if len(keep) == 0:
        return keep
    loc = (R.euler_xyz_matrix(orientation).T @ (env[keep, :3] - pos).T).T
    rng_ = np.sqrt(d2[keep])
    az = np.arctan2(loc[:, 1], loc[:, 0]) * 180 / np.pi
    el = np.arcsin(np.clip(loc[:, 2] / np.maximum(rng_, 1e-6), -1, 1)) * 180 / np.pi
    fov = ((np.abs(az) <= config["fov_horizontal"] / 2) & (np.abs(el) <= config["fov_vertical"] / 2)
           & (rng_ >= config["range_min"]))
    idx = keep[fov]
    cap = config["points_per_frame"]
    if len(idx) > cap:
        idx = idx[np.arange(0, len(idx), len(idx) // cap)[:cap]]
    return idx


def scan_reference(case, config=None):
    """Per frame (oracle64 (n, 4), extended (n, 3), scale): the oracle draws its noise from
    RandomState(SCAN_SEED) in frame order; the extended restatement adds the same draws."""
    cfg = dict(SCAN_CFG if config is None else config)
    r1, r2 = np.random.RandomState(SCAN_SEED), np.random.RandomState(SCAN_SEED)
    out = []
    for k in range(len(case["pos"])):
        ref = R.scan_environment(case["env"], {"position": case["pos"][k], "orientation": case["rpy"][k]}, cfg, rng=r1)
        idx = scan_kept(case["env"], case["pos"][k], case["rpy"][k], cfg)
        assert len(idx) == len(ref)
        noise = r2.normal(0, cfg["lidar_range_noise"], (len(idx), 3)) if len(idx) else np.zeros((0, 3))
        ext = ext_scan_local(case["env"][idx, :3], case["pos"][k], case["rpy"][k], noise)
        out.append((ref, ext, scale_of(case["env"][idx, :3], case["pos"][k])))
    return out


def case_d_ref(frames):
    """d_ref of a case from its per-frame (oracle64, extended, scale)."""
    return max([d_ref(r[:, :3], e, s) for r, e, s in frames] + [0.0])


# One (case, per-frame (oracle64, extended, scale), d_ref) per case and process: computed once, shared
# by the CPU and GPU tests, never modified.
@functools.lru_cache(maxsize=None)
def slerp_bundle(table, pattern):
    case = slerp_case(table, pattern)
    frames = slerp_reference(case)
    return case, frames, case_d_ref(frames)


@functools.lru_cache(maxsize=None)
def imu_bundle(theta_max, pattern):
    case = imu_case(theta_max, pattern)
    frames = imu_reference(case)
    return case, frames, case_d_ref(frames)


@functools.lru_cache(maxsize=None)
def frame_bundle(name):
    case = frame_case(name)
    frames = frame_reference(case)
    return case, frames, case_d_ref(frames)


@functools.lru_cache(maxsize=None)
def affine_bundle(w_column, mats):
    case = affine_case(w_column, mats)
    frames = affine_reference(case)
    return case, frames, case_d_ref(frames)


@functools.lru_cache(maxsize=None)
def scan_bundle():
    case = scan_case()
    frames = scan_reference(case)
    return case, frames, case_d_ref(frames)
