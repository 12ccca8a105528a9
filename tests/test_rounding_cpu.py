"""The "rounded once" bar (tests/rounding.py) without a GPU: it sees the defects it is there for, its
margin is bounded by them, and no GPU case is ill-conditioned.

Mutations: the numpy float64 emulations of slerp_core / imu_core give 0 failures at delta =
MARGIN * d_ref against the float64 oracle; with too short a polynomial for the window's angles, a
float32 alpha, a float32 rotated value, or one wrong coefficient they give more than 0.  60 000
points per case (half random, half cancelling), 180 000 coordinates.
"""
import mpmath
import numpy as np
import pytest

import rounding as Q
from conftest import scale_of
from oracle import restatement as R

N = 60_000


def _mp(v):
    """an extended value as an mpmath number (two float64 pieces)"""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - Q.LD(hi)))


def test_extended_precision_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18
    mpmath.mp.dps = 50
    x = np.array([0.3, 1.45, 31.7, 1e6 + 0.123], dtype=np.float64)
    for v, s, c, a in zip(x, np.sin(x.astype(Q.LD)), np.cos(x.astype(Q.LD)), np.arctan2(x.astype(Q.LD), Q.LD(0.7))):
        assert abs(_mp(s) - mpmath.sin(mpmath.mpf(float(v)))) < 2e-19
        assert abs(_mp(c) - mpmath.cos(mpmath.mpf(float(v)))) < 2e-19
        assert abs(_mp(a) - mpmath.atan2(mpmath.mpf(float(v)), mpmath.mpf(0.7))) < 4e-19


def test_bar_is_an_interval_of_float32_roundings():
    ref = np.array([[1.0 + 2.0 ** -24, 3.0, -2.0]])       # x: a float32 tie
    sc = np.array([1.0])
    up, dn = np.float32(1.0 + 2.0 ** -23), np.float32(1.0)
    assert Q.rounded_once_failures(np.array([[dn, 3.0, -2.0]], np.float32), ref, sc, 0.0) == 0   # tie to even
    assert Q.rounded_once_failures(np.array([[up, 3.0, -2.0]], np.float32), ref, sc, 0.0) == 1
    assert Q.rounded_once_failures(np.array([[up, 3.0, -2.0]], np.float32), ref, sc, 3e-16) == 0  # past the tie
    assert Q.rounded_once_failures(np.array([[np.float32(1.0 + 2.0 ** -22), 3.0, -2.0]], np.float32), ref, sc, 1e-9) == 1
    assert Q.rounded_once_failures(np.array([[np.nan, 3.0, np.float32(-2.0000002)]], np.float32), ref, sc, 1e-12) == 2
    # a cancelling coordinate: the bar is absolute at delta * scale
    ref = np.array([[1e-7, 50.0, 50.0]])
    sc = np.array([100.0])
    y = np.array([[np.float32(1e-7 + 3e-13), 50.0, 50.0]], np.float32)
    assert Q.rounded_once_failures(y, ref, sc, 1e-15) == 1 and Q.rounded_once_failures(y, ref, sc, 4e-15) == 0


def test_cancelling_points_cancel():
    rng = np.random.default_rng(1)
    n = 4000
    M = R.euler_xyz_matrix(rng.uniform(-3, 3, (n, 3)))
    for t in (rng.normal(0, 200.0, (n, 3)), np.zeros((n, 3))):
        p = Q.cancelling_points(M, t, rng)
        assert np.array_equal(p, Q.f32(p))
        c = np.einsum("nij,nj->ni", M, p) + t
        rel = np.abs(c) / scale_of(p, t)[:, None]
        every = ((np.arange(n) // 2) % 2 == 0) & (np.linalg.norm(t, axis=1) >= 1.0)
        assert np.all(rel[every].max(axis=1) < 2e-3)
        assert np.all(rel[~every].min(axis=1) < 2e-3) and np.median(rel[~every].max(axis=1)) > 0.05
        assert np.median(rel.min(axis=1)) < 1e-4


# ----------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------
def _slerp_inputs(theta_lo, theta_hi, seed):
    """One 60 000-point frame over a 100 Hz table of segment angles in (theta_lo, theta_hi]."""
    rng = np.random.default_rng(seed)
    T = 1025
    step = rng.uniform(2 * theta_lo + 0.02, 2 * theta_hi - 0.02, T) * rng.choice([-1.0, 1.0], T)
    yaw = (np.cumsum(step) + np.pi) % (2 * np.pi) - np.pi
    tr = {"time": np.arange(T) * 0.01, "orientation_imu": np.column_stack([rng.normal(0, 0.004, T), rng.normal(0, 0.004, T), yaw]),
          "position_gps": np.array([100.0, -200.0, 5.0]) + np.cumsum(rng.normal(0, 0.3, (T, 3)), axis=0)}
    th = Q.segment_thetas(tr)
    assert theta_lo < th.min() and th.max() <= theta_hi + 0.02
    t_frame = 1.2345
    t_ns = rng.integers(0, 2_000_000_000, N).astype(np.int64)
    Rm, p = R.slerp_pose(tr["time"], tr["position_gps"], tr["orientation_imu"], t_frame + t_ns * 1e-9)
    xyz = Q.mixed_points(Rm, p, rng, N)
    ref = R.deskew_pose_slerp(xyz, t_ns, t_frame, tr)
    sc = scale_of(xyz, p)
    d = Q.d_ref(ref, Q.ext_deskew_pose_slerp(xyz, t_ns, t_frame, tr), sc)
    return (xyz, t_ns, t_frame, tr), ref, sc, d


def _imu_inputs(theta_max, seed, t_max=0.1):
    rng = np.random.default_rng(seed)
    ts, gyro = Q.imu_table(theta_max, "sorted" if t_max == 0.1 else "spread")
    start = int(Q.IMU_STARTS[0])
    t_abs = start + rng.integers(0, int(t_max * 1e9), N).astype(np.int64)
    xyz = Q.mixed_points(Q.imu_rotation(t_abs, start, ts, gyro), np.zeros(3), rng, N)
    ref = R.compensate_arrays(xyz, t_abs, start, ts, gyro)
    sc = scale_of(xyz)
    d = Q.d_ref(ref, Q.ext_compensate_arrays(xyz, t_abs, start, ts, gyro), sc)
    return (xyz, t_abs, start, ts, gyro), ref, sc, d


def _fails(emu, ref, sc, d):
    return Q.rounded_once_failures(emu.astype(np.float32), ref, sc, Q.MARGIN * d)


@pytest.fixture(scope="module")
def slerp_big():
    return _slerp_inputs(0.25, 1.45, 31)


@pytest.fixture(scope="module")
def imu_08():
    return _imu_inputs(0.8, 33)


def test_slerp_emulation_passes_and_short_polynomials_fail(slerp_big):
    a, ref, sc, d = slerp_big
    print(f"slerp big: d_ref {d:.3e}")
    assert d < Q.D_REF_MAX
    assert _fails(Q.emu_slerp(*a, 10), ref, sc, d) == 0
    assert _fails(Q.emu_slerp(*a, "libm"), ref, sc, d) == 0
    assert _fails(Q.emu_slerp(*a, 6), ref, sc, d) > 0          # K = 6 where tier 2 is due
    assert _fails(Q.emu_slerp(*a, 4), ref, sc, d) > 0


def test_slerp_tier1_window_needs_k6():
    a, ref, sc, d = _slerp_inputs(0.2 - 0.02, 0.25 - 0.02, 32)   # Theta in (0.2, 0.25]: tier 1
    print(f"slerp tier 1: d_ref {d:.3e}")
    assert d < Q.D_REF_MAX
    assert _fails(Q.emu_slerp(*a, 6), ref, sc, d) == 0
    assert _fails(Q.emu_slerp(*a, 10), ref, sc, d) == 0
    assert _fails(Q.emu_slerp(*a, 4), ref, sc, d) > 0          # K = 4 where tier 1 is due


def test_slerp_float32_intermediates_and_a_wrong_coefficient_fail(slerp_big):
    a, ref, sc, d = slerp_big
    n = 3 * N
    assert _fails(Q.emu_slerp(*a, 10, alpha32=True), ref, sc, d) > n // 4
    assert _fails(Q.emu_slerp(*a, 10, rot32=True), ref, sc, d) > 0
    # t_frame + t_ns * 1e-9 rounded once (a contracted fma) instead of product then sum: the time moves
    # by an ulp on a few per cent of the points of a 2 s frame (what slerp_time's pragma prevents)
    assert _fails(Q.emu_slerp(*a, 10, fused_time=True), ref, sc, d) > 0
    c, s = Q.poly_coeffs(10)
    c[6] *= 1.01                                               # kPoly10's z^7 term off by 1 %
    assert _fails(Q.emu_slerp(*a, 10, coeffs=(c, s)), ref, sc, d) > 0
    c, s = Q.poly_coeffs(10)
    s[6] *= 1.01
    assert _fails(Q.emu_slerp(*a, 10, coeffs=(c, s)), ref, sc, d) > 0


def test_imu_emulation_passes_and_short_polynomials_fail(imu_08):
    a, ref, sc, d = imu_08
    print(f"imu 0.8: d_ref {d:.3e}")
    assert d < Q.D_REF_MAX
    assert _fails(Q.emu_imu(*a, "libm"), ref, sc, d) == 0
    assert _fails(Q.emu_imu(*a, 10), ref, sc, d) == 0
    assert _fails(Q.emu_imu(*a, 6), ref, sc, d) > 0            # K = 6 where the general tier is due
    assert _fails(Q.emu_imu(*a, "libm", alpha32=True), ref, sc, d) > 0


def test_imu_tier1_window_needs_k6():
    a, ref, sc, d = _imu_inputs(0.24, 34)
    print(f"imu 0.24: d_ref {d:.3e}")
    assert d < Q.D_REF_MAX
    assert _fails(Q.emu_imu(*a, 6), ref, sc, d) == 0
    assert _fails(Q.emu_imu(*a, 4), ref, sc, d) > 0            # K = 4 where tier 1 is due


def test_imu_tier0_window_takes_k4():
    a, ref, sc, d = _imu_inputs(0.0625, 35)
    assert d < Q.D_REF_MAX
    assert _fails(Q.emu_imu(*a, 4), ref, sc, d) == 0


def test_imu_gyro_spike_needs_range_reduction():
    a, ref, sc, d = _imu_inputs(30.0, 36)
    print(f"imu 30: d_ref {d:.3e}")
    assert d < Q.D_REF_MAX
    assert _fails(Q.emu_imu(*a, "libm"), ref, sc, d) == 0
    for K in (4, 6, 10):
        assert _fails(Q.emu_imu(*a, K), ref, sc, d) > 3 * N // 2   # any polynomial at |theta| ~ 30


# ----------------------------------------------------------------------------------------------
# the GPU cases' conditioning
# ----------------------------------------------------------------------------------------------
def test_slerp_tables_hold_their_angle_ranges():
    for kind in Q.SLERP_TABLES:
        tr = Q.pose_table(kind)
        assert len(tr["time"]) <= 4097
        th = Q.segment_thetas(tr)
        lo, hi = Q.THETA_RANGE["small" if kind == "spike" else kind]
        if kind == "spike":
            assert 1.4 < th[Q.SPIKE_ROW] <= 1.45
            th = np.delete(th, Q.SPIKE_ROW)
        assert lo < th.min() and th.max() <= hi, (kind, th.min(), th.max())


@pytest.mark.parametrize("table,pattern", Q.SLERP_CASES)
def test_d_ref_of_slerp_cases(table, pattern):
    case, _, d = Q.slerp_bundle(table, pattern)
    assert max(len(x) for x in case["xyz"]) <= 8192
    print(f"slerp {table}/{pattern}: d_ref {d:.3e}")
    assert 0.0 < d < Q.D_REF_MAX


@pytest.mark.parametrize("theta,pattern", Q.IMU_CASES)
def test_d_ref_of_imu_cases(theta, pattern):
    case, _, d = Q.imu_bundle(theta, pattern)
    assert len(case["ts"]) <= 4097
    # the case's angles are what its name says
    th = np.concatenate([np.abs(R.imu_interpolate_gyro(case["ts"], case["gyro"], case["starts"][f] + t)
                                * (t * 1e-9)[:, None]).max(axis=1) for f, t in enumerate(case["t_ns"]) if len(t)])
    print(f"imu {theta}/{pattern}: d_ref {d:.3e}, max |theta| {th.max():.4f}")
    assert 0.97 * theta < th.max() <= theta
    assert 0.0 < d < Q.D_REF_MAX


@pytest.mark.parametrize("name", Q.FRAME_CASES)
def test_d_ref_of_frame_cases(name):
    d = Q.frame_bundle(name)[2]
    print(f"frame {name}: d_ref {d:.3e}")
    assert 0.0 < d < Q.D_REF_MAX


@pytest.mark.parametrize("w_column,mats", Q.AFFINE_CASES)
def test_d_ref_of_affine_cases(w_column, mats):
    d = Q.affine_bundle(w_column, mats)[2]
    print(f"affine w={w_column}/{mats}: d_ref {d:.3e}")
    assert 0.0 < d < Q.D_REF_MAX


def test_d_ref_of_the_scan_case():
    _, frames, d = Q.scan_bundle()
    assert len(frames) == 4 and sum(len(r) for r, _, _ in frames) > 500
    assert max(len(r) for r, _, _ in frames) == Q.SCAN_CFG["points_per_frame"]    # the subsample is taken
    print(f"scan: d_ref {d:.3e}")
    assert 0.0 < d < Q.D_REF_MAX


# ----------------------------------------------------------------------------------------------
# sincos_prep
# ----------------------------------------------------------------------------------------------
def _sincos_args():
    rng = np.random.default_rng(41)
    x = list(10.0 ** rng.uniform(-3.0, np.log10(2.0 ** 20 * np.pi / 2), 400) * rng.choice([-1.0, 1.0], 400))
    for n in [0, 1, 2, 3, 4, 5, 7, 100, 1001, 65537, 2 ** 19 + 1, 2 ** 20 - 1, 2 ** 20] + list(rng.integers(1, 2 ** 20, 40)):
        for e in (-1e-9, 1e-9):
            x += [int(n) * (np.pi / 2) + e, -(int(n) * (np.pi / 2) + e)]
    return [float(v) for v in x if 1e-3 <= abs(v) <= 2.0 ** 20 * np.pi / 2 + 1e-9]


def _sincos_worst_ulp(parts):
    mpmath.mp.dps = 60
    worst = 0.0
    for v in _sincos_args():
        s, c = Q.sincos_prep(v, parts)
        ms, mc_ = mpmath.sin(mpmath.mpf(v)), mpmath.cos(mpmath.mpf(v))
        ulp = float(np.spacing(max(abs(float(ms)), abs(float(mc_)))))
        worst = max(worst, float(abs(mpmath.mpf(s) - ms)) / ulp, float(abs(mpmath.mpf(c) - mc_)) / ulp)
    return worst


def test_sincos_prep_three_part_reduction_holds_3_ulp():
    """|x| from 1e-3 to 2^20 pi/2, multiples of pi/2 +- 1e-9 included: sin and cos within 3 ulp of
    max(|sin|, |cos|) (kernels.hpp: 2.4 measured); without pio2_3 or without pio2_2 outside."""
    assert len(_sincos_args()) > 500
    w3 = _sincos_worst_ulp((0, 1, 2))
    print(f"sincos_prep: worst {w3:.2f} ulp")
    assert w3 <= 3.0
    assert _sincos_worst_ulp((0, 1)) > 3.0          # pio2_3 dropped
    assert _sincos_worst_ulp((0, 2)) > 3.0          # pio2_2 dropped
