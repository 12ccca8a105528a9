"""GPU scan_environment (csrc/scan.hpp: k_scan_count, k_scan_emit) on its decision edges: the
scenes of tests/scanedges.py, with points ulps from range_min / range_max and 1e-12 .. 1e-2 degrees
from the FOV edges, under rotated and UTM-scale poses, for fast-tier configs and for every kind of
config that disables the fast tier; several poses and two frame groups in one launch on all three
emit paths; the systematic subsample at n = cap, cap + 1, 2 cap - 1, 2 cap, ...

The kept set must be the reference's (scanedges.mask, the oracle's decision) on every row of
scanedges.gpu_asserted: all range decisions, and FOV decisions at least 1e-12 degrees from the edge or
exact by construction.  Rows outside it are reported, never asserted."""
import numpy as np
import pytest

import scanedges as S
from conftest import assert_scaled_close, scale_of
from oracle import codecs as C
from oracle import restatement as R

pytestmark = pytest.mark.gpu

SCENES = [(ci, pi) for ci in range(len(S.CONFIGS)) for pi in range(3)]


def describe(rows, cls, m):
    return [(int(i), S.CLASSES[cls[i]], *(float(m[k][i]) for k in ("az", "el", "rmin", "rmax"))) for i in rows[:8]]


def check_kept(got_ids, keep, m, cls, what):
    """The kept ids equal the reference's, in order, on the gpu_asserted rows; returns (rows outside
    gpu_asserted, those of them decided unlike the reference)."""
    got_ids = np.asarray(got_ids)
    ids = got_ids.astype(np.int64)
    assert np.array_equal(ids, got_ids) and (np.diff(ids) > 0).all(), f"{what}: ids not in scene order"
    want = np.flatnonzero(keep)
    held = S.gpu_asserted(m)
    flipped = np.setxor1d(ids, want)
    outside = flipped[~held[flipped]]
    report = f"{what}: {int((~held).sum())} rows outside gpu_asserted, {len(outside)} of them decided unlike the reference"
    if len(flipped):
        report += (f"; {len(flipped)} rows flipped, {int(held[flipped].sum())} of them asserted; first (id, class, az, el, "
                   f"rmin, rmax margins): {describe(flipped, cls, m)}")
    print(report)
    assert np.array_equal(ids[held[ids]], want[held[want]]), report
    return int((~held).sum()), len(outside)


@pytest.fixture(scope="module")
def many():
    """many_pose_case(ci) with every table pose's reference decision, one config's scene at a time."""
    cache = {}

    def get(ci):
        if ci not in cache:
            env, tr, times, idx = S.many_pose_case(ci)
            cls = np.concatenate([S.edge_scene(ci, pi)[1] for pi in range(3)])
            dec = {}
            for k in np.unique(idx):
                dec[int(k)] = S.mask(env, tr["position_gps"][k], tr["orientation_imu"][k], S.CONFIGS[ci])
            cache.clear()
            cache[ci] = (env, tr, times, idx, cls, dec)
        return cache[ci]
    return get


@pytest.mark.parametrize("ci,pi", SCENES)
def test_edge_scene_kept_set_is_the_reference(mc, gpu_ctx, ci, pi):
    """sim.scan_environment (float64 rows, uncapped, no noise) on one CONFIGS x pose edge scene."""
    cfg = S.CONFIGS[ci]
    pos, rpy = S.poses_of(ci)[pi]
    env, cls = S.edge_scene(ci, pi)
    keep, m = S.mask(env, pos, rpy, cfg)
    sim = mc.LiDARMotionSimulator(S.config_of(cfg), context=gpu_ctx)
    out = sim.scan_environment(env, S.pose_dict(pos, rpy))
    assert out.dtype == np.float64 and out.ndim == 2 and out.shape[1] == 4
    check_kept(out[:, 3], keep, m, cls, f"config {ci} pose {pi}")
    with np.errstate(all="ignore"):
        ref = R.scan_environment(env, S.pose_dict(pos, rpy), sim.config)
    common, io, ir = np.intersect1d(out[:, 3], ref[:, 3], return_indices=True)
    assert len(common) >= int((keep & S.gpu_asserted(m)).sum())
    assert_scaled_close(out[io], ref[ir], scale_of(ref[ir, :3]), what=f"config {ci} pose {pi}")


@pytest.mark.parametrize("ci", range(len(S.CONFIGS)))
def test_many_poses_one_launch_all_emit_paths(mc, gpu_ctx, many, ci):
    """Eight poses, eleven frames (two frame groups, poses selected by next-or-equal) over the three
    poses' edge scenes in one scene: scan_frames (float32 batch), simulate_frames (float64 local and
    aligned) and an emit into a with_pcd_len batch keep the reference's rows per frame; the PCD bytes
    of the with_pcd_len batch are the oracle's for its download."""
    env, tr, times, idx, cls, dec = many(ci)
    sim = mc.LiDARMotionSimulator(S.config_of(S.CONFIGS[ci]), context=gpu_ctx)
    assert len(times) == 11 and len(np.unique(idx)) == 8

    b = sim.scan_frames(env, tr, times)
    frames32 = b.split(b.download_aos())
    res = sim.simulate_frames(env, tr, times)
    counts, _ = gpu_ctx._scan_count(times, sim.config, "searchsorted", np.random)
    pb = gpu_ctx.batch(counts, with_pcd_len=True)
    mc._lib.check(gpu_ctx.lib.mc_scan_emit(gpu_ctx.handle, pb.handle, None), "emit")
    assert pb.pcd_len_current() or counts.sum() == 0      # nothing kept: no emit launch, nothing summed
    host = pb.split(pb.download_aos())
    assert mc.codecs.encode_pcd_batch(pb) == [C.pcd_ascii_bytes(h) for h in host]

    for f, k in enumerate(idx):
        keep, m = dec[int(k)]
        what = f"config {ci} frame {f} (pose {int(k)})"
        check_kept(frames32[f][:, 3], keep, m, cls, what + " float32 batch")
        loc = res["raw_scans"][f]["points_local"]
        al = res["aligned_pointclouds"][f]
        check_kept(loc[:, 3], keep, m, cls, what + " float64 rows")
        assert np.array_equal(loc[:, 3], frames32[f][:, 3]) and np.array_equal(al[:, 3], loc[:, 3]), what
        assert np.array_equal(host[f], frames32[f]), what
        assert counts[f] == len(loc), what
        # the float32 columns are the float64 rows rounded once; the aligned rows are the scene's points
        assert np.array_equal(frames32[f][:, :3], loc[:, :3].astype(np.float32).astype(np.float64)), what
        src = env[loc[:, 3].astype(np.int64), :3]
        scale = scale_of(loc[:, :3], tr["position_gps"][k])
        assert np.all(np.abs(al[:, :3] - src).max(axis=1, initial=0.0) <= 1e-12 * np.maximum(scale, 1e-30)), what


@pytest.mark.parametrize("cap", S.CAPS)
def test_subsample_boundaries(mc, gpu_ctx, cap):
    """cap_scene from the 17 CAP_FRAMES poses in one launch: counts min(cap, ceil(n / (n // cap))), the
    kept ids arange(0, n, n // cap)[:cap] of the visible ids on both emit paths, and with noise the
    global RNG left where the oracle's run leaves it."""
    env, tr = S.cap_scene(), S.CAP_FRAMES
    times = tr["time"]
    cfg = S.config_of(S.CAP_CONFIG, cap)
    sim = mc.LiDARMotionSimulator(cfg, context=gpu_ctx)
    sim._load_environment(env)
    gpu_ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])
    counts, noise = gpu_ctx._scan_count(times, sim.config, "searchsorted", np.random)
    print(f"cap {cap}: counts {counts.tolist()}")
    assert noise is None
    assert counts.tolist() == [S.subsample_count(n, cap) for n in S.CAP_N]
    want = [S.subsample(2.0 * np.arange(S.N_CAP - n, S.N_CAP), cap) for n in S.CAP_N]
    b = gpu_ctx.scan(times, sim.config)
    got32 = b.split(b.download_aos())
    c64, local, _ = gpu_ctx.scan_rows(times, sim.config, aligned=False)
    assert np.array_equal(c64, counts) and np.array_equal(b.counts, counts)
    offs = np.concatenate([[0], np.cumsum(counts)])
    for f, w in enumerate(want):
        assert np.array_equal(got32[f][:, 3], w), (cap, f)
        assert np.array_equal(local[offs[f]:offs[f + 1], 3], w), (cap, f)
    # noise on: the same draws, in frame order, and the generator left in the oracle's state
    noisy = mc.LiDARMotionSimulator(S.config_of(S.CAP_CONFIG, cap, noise=0.02), context=gpu_ctx)
    np.random.seed(77)
    ref = [R.scan_environment(env, S.pose_dict(tr["position_gps"][f], tr["orientation_imu"][f]), noisy.config)
           for f in range(len(times))]
    after = np.random.random()
    np.random.seed(77)
    res = noisy.simulate_frames(env, tr, times)
    assert np.random.random() == after
    for f, r in enumerate(ref):
        out = res["raw_scans"][f]["points_local"]
        assert out.shape == r.shape and np.array_equal(out[:, 3], r[:, 3]), (cap, f)
        assert_scaled_close(out, r, scale_of(r[:, :3]), what=f"cap {cap} frame {f} noisy")
    np.random.seed(77)
    nb = noisy.scan_frames(env, tr, times)
    assert np.random.random() == after and np.array_equal(nb.counts, counts)


def test_points_per_frame_zero_is_rejected_without_a_launch(mc, gpu_ctx):
    """mc_scan_count with points_per_frame 0: MC_ERR_INVALID before anything is launched (the scan
    timing region records one launch for a valid count and none for the rejected one)."""
    lib, ptr = mc._lib, mc._lib.ptr
    env, tr = S.cap_scene(), S.CAP_FRAMES
    gpu_ctx.set_environment(env)
    gpu_ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])
    cfg = S.config_of(S.CAP_CONFIG, 5)
    par = np.array(S.CAP_CONFIG, np.float64)
    t = np.ascontiguousarray(tr["time"])
    counts = np.full(len(t), -7, np.int64)
    gpu_ctx.timing(True)
    try:
        gpu_ctx.read_timing()
        good, _ = gpu_ctx._scan_count(t, cfg, "searchsorted", np.random)
        assert gpu_ctx.read_timing()["scan_launches"] == 1
        for bad in (0, -3):
            rc = gpu_ctx.lib.mc_scan_count(gpu_ctx.handle, len(t), ptr(t, lib.c_double), lib.MC_POSE_SEARCHSORTED,
                                           ptr(par, lib.c_double), bad, ptr(counts, lib.c_int64))
            assert rc == lib.MC_ERR_INVALID, (bad, rc)
        assert gpu_ctx.read_timing()["scan_launches"] == 0
    finally:
        gpu_ctx.timing(False)
    assert (counts == -7).all()
    # the earlier valid count is still the context's state: its emit runs and fills its rows
    n = int(good.sum())
    buf = gpu_ctx.device_buffer(n * 32)
    try:
        assert gpu_ctx.lib.mc_scan_emit_f64(gpu_ctx.handle, None, buf.ptr, None) == lib.MC_OK
        ids = buf.to_host(np.float64, (n, 4))[:, 3]
    finally:
        buf.close()
    want = np.concatenate([S.subsample(2.0 * np.arange(S.N_CAP - k, S.N_CAP), 5) for k in S.CAP_N])
    assert np.array_equal(ids, want)
