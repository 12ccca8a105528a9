"""The float32 batch kernels held to "float64, rounded once" (tests/rounding.py): every output
coordinate must be the float32 rounding of some float64 value within MARGIN * d_ref * (|p| + |t|) of
the float64 oracle (oracle/restatement.py), on float32-valued inputs of which half cancel to ~1e-7 of
their scale.  The 1e-5 bar (conftest.assert_scaled_close) is asserted beside it, unchanged.

Every case prints `case: d_ref ..., worst |out - oracle| / scale ...` (pytest -s); DESIGN §5 records them.
"""
import numpy as np
import pytest

import rounding as Q
from conftest import assert_scaled_close

pytestmark = pytest.mark.gpu


def _rows(xyz, rng_key):
    """(N, 4) rows of the frames' points with an intensity column of float32 values"""
    n = sum(len(x) for x in xyz)
    inten = Q.f32(np.random.default_rng(rng_key).uniform(0.0, 1.0, n))
    return np.column_stack([np.concatenate(xyz), inten])


def _check(what, got, rows, frames, d, counts):
    """got: the (N, 4) download of an output batch; frames: per frame (oracle64, extended, scale)."""
    assert got.shape == rows.shape
    assert np.array_equal(got[:, 3], rows[:, 3]), f"{what}: 4th column not passed through"
    off = np.concatenate([[0], np.cumsum(counts)])
    worst, bad = 0.0, 0
    for f, (ref, _, sc) in enumerate(frames):
        o = got[off[f]:off[f + 1], :3]
        assert_scaled_close(o, ref[:, :3], sc, what=f"{what} frame {f}")
        worst = max(worst, Q.worst_scaled(o, ref[:, :3], sc))
        bad += Q.rounded_once_failures(o, ref[:, :3], sc, Q.MARGIN * d)
    print(f"{what}: d_ref {d:.3e}, worst |out - oracle| / scale {worst:.3e}, outside the bar {bad}")
    assert bad == 0, f"{what}: {bad} coordinates are no float32 rounding within {Q.MARGIN:g} * {d:.2e} * scale of the oracle"


def _all_outputs(ctx, b, counts, mode, select="searchsorted"):
    """The batch deskewed out of place into a plain batch, into a with_pcd_len batch, through
    deskew_steps (the fused next-prep kernels) and in place: bit-equal; returns the download."""
    got = ctx.deskew(b, ctx.batch(counts), mode=mode, pose_select=select).download_aos()
    pcd = ctx.deskew(b, ctx.batch(counts, with_pcd_len=True), mode=mode, pose_select=select).download_aos()
    assert np.array_equal(pcd.view(np.uint64), got.view(np.uint64)), "with_pcd_len output differs"
    steps = ctx.deskew_steps(b, ctx.batch(counts), 2, mode=mode, pose_select=select).download_aos()
    assert np.array_equal(steps.view(np.uint64), got.view(np.uint64)), "deskew_steps output differs"
    ctx.deskew(b, b, mode=mode, pose_select=select)
    assert np.array_equal(b.download_aos().view(np.uint64), got.view(np.uint64)), "in-place output differs"
    return got


@pytest.mark.parametrize("table,pattern", Q.SLERP_CASES)
def test_slerp_rounded_once(gpu_ctx, table, pattern):
    """k_deskew_points<1>: 100 Hz tables of segment angles in (0, 1/16], (1/16, 1/4], (1/4, 1.45] and
    one 1.45 segment among small ones; time-sorted frames (SGPR path, sub-tiles across a segment
    boundary), shuffled over 10 segments (LDS window), spread over 3 s (per-point search), and
    ("far") sub-tile windows outside k_prep's probe window."""
    case, frames, d = Q.slerp_bundle(table, pattern)
    tr = case["tr"]
    gpu_ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])
    rows = _rows(case["xyz"], 1)
    b = gpu_ctx.batch(Q.COUNTS, with_time=True)
    b.upload_aos(rows)
    b.upload_time(np.concatenate(case["t_ns"]))
    b.set_frame_times(case["times"])
    got = _all_outputs(gpu_ctx, b, Q.COUNTS, "pose_slerp")
    _check(f"slerp {table}/{pattern}", got, rows, frames, d, Q.COUNTS)


@pytest.mark.parametrize("theta,pattern", Q.IMU_CASES)
def test_imu_rounded_once(gpu_ctx, theta, pattern):
    """k_deskew_points<2>: a 200 Hz table whose rates put max |theta| just below and above 1/16 and
    1/4, at 0.8 and at 30 (range reduction), a rate flip between two samples; the SLERP time patterns."""
    case, frames, d = Q.imu_bundle(theta, pattern)
    gpu_ctx.set_imu(case["ts"], case["gyro"])
    rows = _rows(case["xyz"], 2)
    b = gpu_ctx.batch(Q.COUNTS, with_time=True)
    b.upload_aos(rows)
    b.upload_time(np.concatenate(case["t_ns"]))
    b.set_frame_starts(case["starts"])
    got = _all_outputs(gpu_ctx, b, Q.COUNTS, "imu")
    _check(f"imu {theta}/{pattern}", got, rows, frames, d, Q.COUNTS)


@pytest.mark.parametrize("name", Q.FRAME_CASES)
def test_frame_mode_rounded_once(gpu_ctx, name):
    """k_deskew_frame with k_prep's Euler -> R through sincos_prep: angles of order 1, 1e3, 1e6 rad, at
    multiples of pi/2 +- 1e-9, translations of 5e5 m; both pose selections."""
    case, frames, d = Q.frame_bundle(name)
    gpu_ctx.set_trajectory(case["time"], case["pos"], case["rpy"])
    rows = _rows(case["xyz"], 3)
    b = gpu_ctx.batch(Q.FRAME_COUNTS)
    b.upload_aos(rows)
    b.set_frame_times(case["ftimes"])
    got = _all_outputs(gpu_ctx, b, Q.FRAME_COUNTS, "frame", case["select"])
    _check(f"frame {name}", got, rows, frames, d, Q.FRAME_COUNTS)


@pytest.mark.parametrize("w_column,mats", Q.AFFINE_CASES)
def test_transform_affine_rounded_once(gpu_ctx, w_column, mats):
    """transform_affine on a batch (w_column: k_affine_w), one matrix and one per frame, a UTM-scale
    translation among them."""
    case, frames, d = Q.affine_bundle(w_column, mats)
    rows = np.column_stack([np.concatenate(case["xyz"]), np.concatenate(case["w"])])
    b = gpu_ctx.batch(Q.FRAME_COUNTS)
    b.upload_aos(rows)
    M = case["M"][0] if mats == "one" else case["M"]
    got = gpu_ctx.transform_affine(b, gpu_ctx.batch(Q.FRAME_COUNTS), M, w_column=w_column).download_aos()
    _check(f"affine w={w_column}/{mats}", got, rows, frames, d, Q.FRAME_COUNTS)
    gpu_ctx.transform_affine(b, b, M, w_column=w_column)
    assert np.array_equal(b.download_aos().view(np.uint64), got.view(np.uint64)), "in-place output differs"


def _stager_rows(n, ld, seed):
    """float64 rows whose float32 rounding is exercised: random magnitudes over the whole float32
    range and beyond, ties to even, overflow to +-inf, float32 subnormals, +-0.0, NaN."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 1.0, (n, ld)) * 10.0 ** rng.uniform(-50.0, 42.0, (n, ld))
    f = (rng.normal(0.0, 1.0, 64) * 10.0 ** rng.uniform(-44.0, 38.0, 64)).astype(np.float32)
    f = f[np.isfinite(f)]
    nxt = np.nextafter(f, np.float32(np.inf))
    ties = 0.5 * (f.astype(np.float64) + nxt.astype(np.float64))          # exact midpoints, subnormal ones too
    fmax = float(np.finfo(np.float32).max)
    sub = 2.0 ** -149
    special = np.concatenate([ties, -ties, np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf), [
        0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, fmax, -fmax, fmax + 2.0 ** 103, -(fmax + 2.0 ** 103),
        np.nextafter(fmax + 2.0 ** 103, 0.0), 1e39, -1e39, 1e300, -1e300, sub, -sub, 0.5 * sub, -0.5 * sub,
        np.nextafter(0.5 * sub, 1.0), 1.5 * sub, 2.5 * sub, 1e-40, -1e-40, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0),
        5e-324, 1e-300]])
    pos = rng.choice(n * ld, len(special), replace=False)
    a.ravel()[pos] = special
    return a


def _same_float32_bits(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("ld", [4, 6])
def test_stager_rounds_to_nearest_even(gpu_ctx, ld):
    """stage_aos_device and upload_aos of arbitrary float64 rows equal astype(float32) bit for bit."""
    counts = np.array([255, 256, 257])
    n = int(counts.sum())
    rows = _stager_rows(n, ld, 50 + ld)
    with np.errstate(over="ignore"):
        want = rows[:, :4].astype(np.float32)
    assert np.isinf(want).sum() > 8 and np.isnan(want).sum() >= 2 and (want == 0).sum() > 4
    b = gpu_ctx.batch(counts)
    b.upload_aos(rows)
    for c, col in enumerate(b.download_columns()):
        assert _same_float32_bits(col, want[:, c]), f"upload_aos ld {ld} column {c}"
    buf = gpu_ctx.device_buffer(rows.nbytes)
    buf.from_host(rows)
    b2 = gpu_ctx.batch(counts)
    b2.stage_aos_device(buf, ld=ld)
    for c, col in enumerate(b2.download_columns()):
        assert _same_float32_bits(col, want[:, c]), f"stage_aos_device ld {ld} column {c}"


def test_scan_batch_rounded_once(gpu_ctx):
    """scan into a float32 batch with range noise on: float32(oracle visible + noise) under the bar."""
    case, frames, d = Q.scan_bundle()
    gpu_ctx.set_environment(case["env"])
    gpu_ctx.set_trajectory(np.arange(4.0), case["pos"], case["rpy"])
    b = gpu_ctx.scan(np.arange(4.0), dict(Q.SCAN_CFG), pose_select="direct", rng=np.random.RandomState(Q.SCAN_SEED))
    counts = [len(r) for r, _, _ in frames]
    assert b.counts.tolist() == counts
    rows = np.vstack([r for r, _, _ in frames])
    _check("scan", b.download_aos(), rows, frames, d, counts)
