"""GPU: k_prep's pose and IMU table searches on non-uniform time tables (timetables.py).

k_prep decides a frame's place in the pose / IMU table from the 64 entries around an interpolation
guess (kernels.hpp probe_base / probe_count) and takes the wave-cooperative full search
(wave_count<true>, wave_count2<false>) only when that window does not decide.  Every other GPU test
uploads a uniform grid, where the guess is right.  Here the guess misses for most frames: curved,
bursty and dropout tables, runs of equal timestamps around the window's 64 entries (ties resolve
'left' for Path A, 'right' - 1 for SLERP and the IMU), a table of one value, tables of 65...129
entries (the window clamped at n - 64), of 4096 / 4097 (a second search round) and of 20011 (a
third).  Pose sequences with isolated large segment angles catch a polynomial tier taken from a
neighbouring segment.  Each case also runs as two pipelined steps (the copy of the prep inside the
deskew kernels) and through the float64 row path; all against the oracle at the parity bar.
"""
import numpy as np
import pytest

import timetables as tt
from conftest import assert_scaled_close, scale_of
from oracle import restatement as R

pytestmark = pytest.mark.gpu

COUNTS = (5000, 3, 256, 1024, 1025)
GUARD_NS = 1500          # points keep at least this from a repeated timestamp (asserted: >= 1 us)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _cols(b):
    return np.stack(b.download_columns())


def _t_ns(rng, regime, n):
    """The fuzz's point-time regimes: a sorted 100 ms frame, a shuffled one, seconds either side of
    the frame time, a sorted +-3 ms around it."""
    if regime == 0:
        return np.sort(rng.integers(0, 100_000_000, n)).astype(np.int64)
    if regime == 1:
        return rng.integers(0, 100_000_000, n).astype(np.int64)
    if regime == 2:
        return rng.integers(-1_500_000_000, 1_500_000_000, n).astype(np.int64)
    return np.sort(rng.integers(-3_000_000, 3_000_000, n)).astype(np.int64)


def _frames(rng, F):
    """F frames: counts cycling through COUNTS, every count with every regime; float32-valued points."""
    counts = np.array([COUNTS[i % 5] for i in range(F)])
    regimes = [(i // 5 + i) % 4 for i in range(F)]
    pts = [f32(np.column_stack([rng.uniform(-90, 90, (n, 3)), rng.uniform(0, 1, n)])) for n in counts]
    t_ns = [_t_ns(rng, r, n) for r, n in zip(regimes, counts)]
    return counts, pts, t_ns


def _frame_times(rng, time, F):
    """Frame times over the whole table, both ends included: half uniform in time (long gaps), half
    at table entries (dense stretches too)."""
    k = rng.integers(0, len(time), F // 2)
    t = np.concatenate([[time[0], time[-1]], rng.uniform(time[0] - 0.05, time[-1] + 0.05, F - F // 2 - 2),
                        time[k] + rng.uniform(-0.01, 0.01, F // 2)])
    return rng.permutation(t)


# ---------------------------------------------------------------------------------------------
# a. Path A: the pose index (LMC:804-812)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,T", [(k, T) for k in tt.KINDS for T in tt.SIZES] + [("flat", tt.FLAT_T)])
def test_frame_mode_pose_index_on_nonuniform_tables(mc, gpu_ctx, kind, T):
    """One small frame per query time, point 0 at the origin and pos[k] = (k, -2k, 0.5k): the
    origin's image names the pose the kernel chose.  It must be numpy's searchsorted 'left', clamped
    (a NaN frame time sorts last: the last pose), on the float32 batch path, after two pipelined
    steps (byte equal) and on the float64 row path."""
    time = tt.table(kind, T, tt.SEED)
    pos, rpy = tt.poses(T, tt.SEED, spiky=False)
    tr = {"time": time, "position_gps": pos, "orientation_imu": rpy}
    q = tt.frame_queries(kind, time)
    F = len(q)
    share = float(tt.guess_misses(time, q).mean())
    print(f"guess_misses share {kind} T={T}: {share:.3f} of {F} frames")
    if T >= 4096:
        assert share >= 0.5, "the inputs no longer leave the probe window: change the generator"
    rng = np.random.default_rng([T, 21])
    counts = rng.integers(1, 6, F)
    offs = np.concatenate([[0], np.cumsum(counts)])
    aos = f32(np.column_stack([rng.uniform(-90, 90, (offs[-1], 3)), rng.uniform(0, 1, offs[-1])]))
    aos[offs[:-1], :3] = 0.0
    want = R.select_pose_index(time, q)
    nan = np.flatnonzero(np.isnan(q))
    assert nan.size == 1 and want[nan[0]] == T - 1                     # numpy: NaN sorts last
    ref = np.concatenate([R.transform_pointcloud(aos[offs[f]:offs[f + 1]],
                                                 {"translation": pos[k], "rotation": rpy[k]})
                          for f, k in enumerate(want)])
    sc = scale_of(aos[:, :3]) + np.repeat(np.linalg.norm(pos[want], axis=1), counts)

    def decoded(xyz0):
        k = np.rint(xyz0[:, 0]).astype(np.int64)
        assert np.array_equal(xyz0, np.column_stack([k, -2.0 * k, 0.5 * k])), "point 0 is no pose's position"
        return k

    def same_index(got, path):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{path}: {bad.size} of {F} frames took another pose; first: frame time "
                               f"{q[bad[0]]!r} got {got[bad[0]]} want {want[bad[0]]}")

    gpu_ctx.set_trajectory(time, pos, rpy)
    b = gpu_ctx.batch(counts)
    b.upload_aos(aos)
    b.set_frame_times(q)
    out = gpu_ctx.deskew(b, mode="frame")
    got = out.download_aos()
    same_index(decoded(got[offs[:-1], :3]), "batch")
    worst = assert_scaled_close(got[:, :3], ref[:, :3], sc, what=f"batch {kind} T={T}")
    assert np.array_equal(got[:, 3], aos[:, 3])
    # two pipelined steps: the second step's prep runs inside the first step's deskew kernel
    out2 = gpu_ctx.batch(counts)
    gpu_ctx.deskew_steps(b, out2, 2, mode="frame")
    gpu_ctx.sync()
    assert np.array_equal(_cols(out2), _cols(out))
    # float64 rows: the host's pose selection (rot.cpp frame_poses)
    sim = mc.LiDARMotionSimulator(context=gpu_ctx)
    rows = np.concatenate(sim.run_alignment([aos[offs[f]:offs[f + 1]] for f in range(F)], tr, q))
    same_index(decoded(rows[offs[:-1], :3]), "float64 rows")
    worst64 = assert_scaled_close(rows[:, :3], ref[:, :3], sc, what=f"float64 rows {kind} T={T}")
    print(f"worst scaled error {kind} T={T}: batch {worst:.2e}, float64 rows {worst64:.2e}")
    for x in (out, out2, b):
        x.close()


# ---------------------------------------------------------------------------------------------
# b. SLERP: the segment window and its tier
# ---------------------------------------------------------------------------------------------
def _keep_clear(t_ns, base, values):
    """Move every point of t_ns (ns, relative to ``base``: a float frame time in s or an int start in
    ns) that lies within GUARD_NS of one of ``values`` (same unit as base) to GUARD_NS after it; a
    sorted frame stays sorted."""
    for v in values:
        if isinstance(base, float):
            d = np.abs((base + t_ns * 1e-9) - v) * 1e9
            at = int(np.ceil((v - base) * 1e9))
        else:
            d = np.abs(base + t_ns - v)
            at = int(v - base)
        t_ns[d < GUARD_NS] = at + GUARD_NS
    return t_ns


def _tier_frames(time, rpy, avoid, most=4):
    """Frames that pair a quiet segment with a large one in one two-segment window, all points of
    both segments covered (alpha up to 1 in each), so that a sin / cos polynomial tier taken from one
    of the two segments alone is grossly wrong on the other.  For up to ``most`` segments s with
    Theta > 0.5 whose neighbours s - 1, s + 1, s + 2 have Theta < 0.0625 (kernels.hpp kTier0):
      256 points over segments [s - 1, s], 256 over [s, s + 1]      (frame windows of two segments)
      1024 over [s - 1, s] then 1024 over [s + 1, s + 2]           (a four-segment frame: sub-tile
                                                                    windows of two segments each)
    Points are sorted integer ns, 2 ns inside their segments' ends; segments in or next to a run of
    equal timestamps (``avoid``: sample indices) are not used.  Returns (frame times, [t_ns])."""
    q = R.euler_xyz_quat(rpy)
    th = np.arccos(np.minimum(np.abs(np.sum(q[:-1] * q[1:], axis=1)), 1.0))     # Theta of segment k
    T = len(time)
    bad = np.zeros(T + 4, bool)
    for k in avoid:
        bad[max(k - 3, 0):k + 4] = True
    times, t_ns = [], []
    for s in np.flatnonzero(th > 0.5):
        if s < 1 or s + 3 > T - 1 or bad[s] or max(th[s - 1], th[s + 1], th[s + 2]) >= 0.0625:
            continue
        if time[s + 3] - time[s - 1] > 2.0 or len(times) >= 3 * most:
            continue
        tf = float(time[s - 1])

        def span(a, b, n):      # n sorted points inside [time[a], time[b])
            lo = int(np.ceil((time[a] - tf) * 1e9)) + 2
            hi = int(np.floor((time[b] - tf) * 1e9)) - 2
            return np.linspace(lo, hi, n).astype(np.int64)

        for t in (span(s - 1, s + 1, 256), span(s, s + 2, 256),
                  np.concatenate([span(s - 1, s + 1, 1024), span(s + 1, s + 3, 1024)])):
            k = np.searchsorted(time, tf + t * 1e-9, "right") - 1
            assert k.min() == (s if len(t_ns) % 3 == 1 else s - 1) and k.max() == k.min() + (3 if len(t) == 2048 else 1)
            times.append(tf)
            t_ns.append(t)
    return times, t_ns


@pytest.mark.parametrize("T", [129, 4097, 20011])
@pytest.mark.parametrize("kind", tt.KINDS)
def test_slerp_on_nonuniform_tables(mc, gpu_ctx, kind, T):
    """40 frames of 3...5000 points over the whole table, in the fuzz's four point-time regimes: with
    gaps from 10 us to 1 s a frame spans 1 to ~1e4 segments (SGPR records, per-sub-tile windows, the
    LDS window, the out-of-line search).  plateaus: no point within 1 us of a repeated timestamp,
    except one point per run placed exactly on it (frame time = the timestamp, t_ns = 0: exact on
    both sides), which must come out as the run's last sample.  Then _tier_frames: the windows whose
    tier must come from the larger of two very different segments."""
    time = tt.table(kind, T, tt.SEED)
    pos, rpy = tt.poses(T, tt.SEED, spiky=True)
    tr = {"time": time, "position_gps": pos, "orientation_imu": rpy}
    rng = np.random.default_rng([T, 22])
    counts, pts, t_ns = _frames(rng, 40)
    times = _frame_times(rng, time, 40)
    runs = tt.plateau_runs(T) if kind == "plateaus" else []
    run_t = [float(time[s]) for s, _ in runs]
    t_ns = [_keep_clear(t, float(tf), run_t) for t, tf in zip(t_ns, times)]
    for v in run_t:                                        # the points exactly on a repeated timestamp
        pts.append(f32(np.column_stack([rng.uniform(-90, 90, (3, 3)), rng.uniform(0, 1, 3)])))
        t_ns.append(np.array([0, 3_000_000, -3_000_000], np.int64))
        times = np.append(times, v)
        counts = np.append(counts, 3)
    tier_tf, tier_t = _tier_frames(time, rpy, [k for s, n in runs for k in range(s, s + n)])
    assert T < 4097 or len(tier_tf) >= 6, "no quiet / large segment pairs: change the generator"
    for tf, t in zip(tier_tf, tier_t):                      # two-segment windows, quiet beside large
        pts.append(f32(np.column_stack([rng.uniform(-90, 90, (len(t), 3)), rng.uniform(0, 1, len(t))])))
        t_ns.append(t)
        times = np.append(times, tf)
        counts = np.append(counts, len(t))
    F = len(counts)
    offs = np.concatenate([[0], np.cumsum(counts)])
    aos, tt_all = np.concatenate(pts), np.concatenate(t_ns)
    tq = np.repeat(times, counts) + tt_all * 1e-9           # as the oracle forms each point's time
    on_run = np.zeros(len(tq), bool)
    on_run[offs[40:40 + len(runs)]] = True
    for v in run_t:
        assert np.all(np.abs(tq[~on_run] - v) >= 1e-6) and np.count_nonzero(tq[on_run] == v) == 1
    ref = np.concatenate([R.deskew_pose_slerp(pts[f][:, :3], t_ns[f], times[f], tr) for f in range(F)])
    _, pp = R.slerp_pose(time, pos, rpy, tq)
    sc = scale_of(aos[:, :3], pp)
    for r, (s, n) in enumerate(runs):                       # the run's last sample, stated directly
        i = offs[40 + r]
        last = R.transform_pointcloud(aos[i:i + 1], {"translation": pos[s + n - 1], "rotation": rpy[s + n - 1]})
        assert_scaled_close(ref[i:i + 1], last[:, :3], sc[i:i + 1], what=f"oracle at run {r}")

    gpu_ctx.set_trajectory(time, pos, rpy)
    b = gpu_ctx.batch(counts, with_time=True)
    b.upload_aos(aos)
    b.upload_time(tt_all.astype(np.int32))
    b.set_frame_times(times)
    out = gpu_ctx.deskew(b, mode="pose_slerp")
    got = out.download_aos()
    out2 = gpu_ctx.batch(counts, with_time=True)
    gpu_ctx.deskew_steps(b, out2, 2, mode="pose_slerp")
    gpu_ctx.sync()
    steps_equal = np.array_equal(_cols(out2), _cols(out))
    sim = mc.LiDARMotionSimulator(context=gpu_ctx)
    rows = np.concatenate(sim.deskew_frames(pts, t_ns, tr, times))
    for x in (out, out2, b):
        x.close()
    for path, o in (("batch", got), ("float64 rows", rows)):
        worst = 0.0
        for f in range(F):
            s = slice(offs[f], offs[f + 1])
            worst = max(worst, assert_scaled_close(o[s, :3], ref[s], sc[s],
                                                   what=f"{path} {kind} T={T} frame {f} ({counts[f]} pts)"))
        print(f"worst scaled error {kind} T={T} {path}: {worst:.2e}")
        assert np.array_equal(o[:, 3], aos[:, 3])
    assert steps_equal, "two pipelined steps differ from the plain call"


# ---------------------------------------------------------------------------------------------
# c. IMU: a table past 4096 samples, runs of equal timestamps longer than the window
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bursty", "plateaus"])
def test_imu_on_long_and_repeated_timestamp_tables(mc, gpu_ctx, kind):
    """M = 20011 IMU samples (three search rounds) at bursty / plateau timestamps, a spiky gyro,
    20 frames in the four point-time regimes; plateaus: no point within 1 us of a repeated timestamp
    except one per run placed exactly on it (7 ms into its frame, so that its angle is not zero)."""
    M = 20011
    ts = np.round(tt.table(kind, M, tt.SEED) * 1e9).astype(np.int64)
    assert np.all(np.diff(ts) >= 0)
    rng = np.random.default_rng([M, 23])
    gyro = rng.normal(0, 0.5, (M, 3))
    gyro[rng.integers(0, M, 3)] *= 200.0
    counts, pts, t_ns = _frames(rng, 20)
    starts = np.round(_frame_times(rng, ts * 1e-9, 20) * 1e9).astype(np.int64)
    runs = tt.plateau_runs(M) if kind == "plateaus" else []
    run_t = [int(ts[s]) for s, _ in runs]
    t_ns = [_keep_clear(t, int(s0), run_t) for t, s0 in zip(t_ns, starts)]
    for v in run_t:
        pts.append(f32(np.column_stack([rng.uniform(-90, 90, (3, 3)), rng.uniform(0, 1, 3)])))
        t_ns.append(np.array([7_000_000, 0, 20_000_000], np.int64))
        starts = np.append(starts, v - 7_000_000)
        counts = np.append(counts, 3)
    F = len(counts)
    offs = np.concatenate([[0], np.cumsum(counts)])
    aos, tt_all = np.concatenate(pts), np.concatenate(t_ns)
    t_abs = np.repeat(starts, counts) + tt_all
    on_run = np.zeros(len(t_abs), bool)
    on_run[offs[20:F]] = True
    for v in run_t:
        assert np.all(np.abs(t_abs[~on_run] - v) >= 1000) and np.count_nonzero(t_abs[on_run] == v) == 1

    gpu_ctx.set_imu(ts, gyro)
    b = gpu_ctx.batch(counts, with_time=True)
    b.upload_aos(aos)
    b.upload_time(tt_all.astype(np.int32))
    b.set_frame_starts(starts)
    out = gpu_ctx.deskew(b, mode="imu")
    got = out.download_aos()
    out2 = gpu_ctx.batch(counts, with_time=True)
    gpu_ctx.deskew_steps(b, out2, 2, mode="imu")
    gpu_ctx.sync()
    steps_equal = np.array_equal(_cols(out2), _cols(out))
    for x in (out, out2, b):
        x.close()
    worst = 0.0
    for f in range(F):
        s = slice(offs[f], offs[f + 1])
        ref = R.compensate_arrays(aos[s, :3], starts[f] + t_ns[f], starts[f], ts, gyro)
        worst = max(worst, assert_scaled_close(got[s, :3], ref, scale_of(aos[s, :3]),
                                               what=f"imu {kind} frame {f} ({counts[f]} pts)"))
    print(f"worst scaled error imu {kind}: {worst:.2e}")
    assert np.array_equal(got[:, 3], aos[:, 3])
    assert steps_equal, "two pipelined steps differ from the plain call"
