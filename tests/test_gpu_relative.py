"""The relative (sensor-frame) SLERP deskew on the device (mc_deskew_relative, mc_deskew_points_relative_f64,
mc_pose_at, mc_batch_time_spans), held to "float64, rounded once" (tests/relative.py):

    p' = R_ref^T ( R(q(t)) p + pos(t) - pos_ref ),  (R_ref, pos_ref) = slerp_pose(table, t_ref[f])

Every batch output coordinate must be the float32 rounding of some float64 value within
MARGIN * d_ref * (|p| + |pos(t)| + |pos_ref|) of the float64 oracle, on pose tables as generated and
shifted to UTM scale, with half of the points cancelling in the reference frame; the 1e-5 bar
(conftest.assert_scaled_close) is asserted beside it.

Every case prints `case: d_ref ..., worst |out - oracle| / scale ...` (pytest -s); DESIGN §5 records them.
"""
import numpy as np
import pytest

import relative as V
import rounding as Q
from conftest import assert_scaled_close
from oracle import restatement as R

pytestmark = pytest.mark.gpu


def _rows(case, key=1):
    n = sum(len(x) for x in case["xyz"])
    inten = Q.f32(np.random.default_rng(key).uniform(0.0, 1.0, n))
    return np.column_stack([np.concatenate(case["xyz"]), inten])


def _batch(ctx, case, rows):
    b = ctx.batch(Q.COUNTS, with_time=True)
    b.upload_aos(rows)
    b.upload_time(np.concatenate(case["t_ns"]))
    b.set_frame_times(case["times"])
    return b


def _ref_arg(ref):
    return V.KEYFRAME_T if ref == "key" else ref


def _set_table(ctx, tr):
    ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])


def _bar(what, got, frames, d):
    """got (N, >=3) against the per-frame (oracle64, extended, scale): the 1e-5 gate and the bar."""
    off = np.concatenate([[0], np.cumsum(Q.COUNTS)])
    worst, bad = 0.0, 0
    for f, (ref, _, sc) in enumerate(frames):
        o = got[off[f]:off[f + 1], :3]
        assert_scaled_close(o, ref, sc, what=f"{what} frame {f}")
        worst = max(worst, Q.worst_scaled(o, ref, sc))
        bad += Q.rounded_once_failures(o, ref, sc, Q.MARGIN * d)
    print(f"{what}: d_ref {d:.3e}, worst |out - oracle| / scale {worst:.3e}, outside the bar {bad}")
    assert bad == 0, f"{what}: {bad} coordinates are no float32 rounding within {Q.MARGIN:g} * {d:.2e} * scale of the oracle"


@pytest.mark.parametrize("table,pattern,shifted,ref", V.CASES)
def test_relative_rounded_once(mc, gpu_ctx, table, pattern, shifted, ref):
    case, frames, d = V.relative_bundle(table, pattern, shifted, ref)
    what = f"relative {table}/{pattern}/{'shifted' if shifted else 'as generated'}/{ref}"
    _set_table(gpu_ctx, case["tr"])
    rows = _rows(case)
    t_ns = np.concatenate(case["t_ns"])
    b = _batch(gpu_ctx, case, rows)
    used = gpu_ctx.reference_times(b, _ref_arg(ref))
    assert (used is None) if ref == "start" else np.array_equal(used, case["t_ref"])
    out = gpu_ctx.deskew(b, gpu_ctx.batch(Q.COUNTS, with_time=True), mode="pose_slerp", reference=_ref_arg(ref))
    got = out.download_aos()
    assert np.array_equal(got[:, 3].view(np.uint64), rows[:, 3].view(np.uint64)), "intensity not passed through"
    assert np.array_equal(out.download_time(), t_ns), "t_ns not passed through"
    _bar(what, got, frames, d)
    # the float64 rows by the direct formula: the oracle at the float64 SLERP rows' tolerance, and an
    # independent device-side reference the batch output passes the bar against
    o64 = mc.runtime.deskew_points_f64(gpu_ctx, "pose_slerp", Q.COUNTS, rows, t_ns, frame_times=case["times"],
                                       t_ref=case["t_ref"])
    assert np.array_equal(o64[:, 3], rows[:, 3])
    off = np.concatenate([[0], np.cumsum(Q.COUNTS)])
    bad = 0
    for f, (oracle, _, sc) in enumerate(frames):
        s = slice(off[f], off[f + 1])
        assert_scaled_close(o64[s, :3], oracle, sc, what=f"{what} float64 rows frame {f}")
        bad += Q.rounded_once_failures(got[s, :3], o64[s, :3], sc, Q.MARGIN * d)
    assert bad == 0, f"{what}: {bad} batch coordinates outside the bar around the float64 rows"
    # in place
    gpu_ctx.deskew(b, b, mode="pose_slerp", reference=_ref_arg(ref))
    assert np.array_equal(b.download_aos().view(np.uint64), got.view(np.uint64)), "in-place output differs"
    assert np.array_equal(b.download_time(), t_ns)
    if ref == "end":
        # the last return of every non-empty frame is at the reference time: it maps to itself
        for f, n in enumerate(Q.COUNTS):
            if n:
                j = int(np.argmax(case["t_ns"][f]))
                s = slice(off[f] + j, off[f] + j + 1)
                assert Q.rounded_once_failures(got[s, :3], rows[s, :3], frames[f][2][j:j + 1], Q.MARGIN * d) == 0, f


def _frame_refs(case, t_ref):
    """Per frame (oracle64, extended, scale) of case's points for other reference times, and d_ref."""
    frames = V.relative_reference(dict(case, t_ref=t_ref))
    return frames, Q.case_d_ref(frames)


def test_global_unchanged_and_table_rebuilt(gpu_ctx):
    """reference=None is bit-equal to the global deskew before and after relative calls on the same batch
    and context (speculated calls included); relative calls with other reference times, another
    trajectory and other frame times on one batch each give their own result (the cached table is rebuilt)."""
    case, frames, d = V.relative_bundle("big", "sorted", True, "start")
    _set_table(gpu_ctx, case["tr"])
    rows = _rows(case)
    b = _batch(gpu_ctx, case, rows)
    o = gpu_ctx.batch(Q.COUNTS, with_time=True)
    bits = lambda a: a.view(np.uint64)
    g0 = gpu_ctx.deskew(b, o, mode="pose_slerp").download_aos()
    for _ in range(2):   # an identical call speculates the next one's prep; the one after finds it ready
        assert np.array_equal(bits(gpu_ctx.deskew(b, o, mode="pose_slerp").download_aos()), bits(g0))
    gpu_ctx.deskew(b, o, mode="pose_slerp")           # leaves a speculated table half behind
    r0 = gpu_ctx.deskew(b, gpu_ctx.batch(Q.COUNTS, with_time=True), mode="pose_slerp", reference="start").download_aos()
    _bar("start", r0, frames, d)
    for _ in range(3):
        assert np.array_equal(bits(gpu_ctx.deskew(b, o, mode="pose_slerp").download_aos()), bits(g0))
    # the same reference again: the cached table
    r1 = gpu_ctx.deskew(b, o, mode="pose_slerp", reference="start").download_aos()
    assert np.array_equal(bits(r1), bits(r0))
    # other reference times
    t_key = np.full(len(Q.COUNTS), V.KEYFRAME_T)
    fk, dk = _frame_refs(case, t_key)
    _bar("key after start", gpu_ctx.deskew(b, o, mode="pose_slerp", reference=V.KEYFRAME_T).download_aos(), fk, dk)
    t_mix = case["times"] + np.array([0.05, -0.3, 0.0, 2.0, 0.01, -0.02])
    fm, dm = _frame_refs(case, t_mix)
    _bar("per-frame times", gpu_ctx.deskew(b, o, mode="pose_slerp", reference=t_mix).download_aos(), fm, dm)
    _bar("start again", gpu_ctx.deskew(b, o, mode="pose_slerp", reference="start").download_aos(), frames, d)
    # another trajectory, the same reference
    tr2 = dict(case["tr"], position_gps=case["tr"]["position_gps"] - V.SHIFT)
    _set_table(gpu_ctx, tr2)
    f2, d2 = _frame_refs(dict(case, tr=tr2), case["t_ref"])
    _bar("other trajectory", gpu_ctx.deskew(b, o, mode="pose_slerp", reference="start").download_aos(), f2, d2)
    # other frame times ("start" follows them)
    times3 = case["times"] + 0.5
    b.set_frame_times(times3)
    f3, d3 = _frame_refs(dict(case, tr=tr2, times=times3), times3)
    _bar("other frame times", gpu_ctx.deskew(b, o, mode="pose_slerp", reference="start").download_aos(), f3, d3)
    assert np.array_equal(bits(b.download_aos()), bits(rows)), "the input batch changed"


def test_one_pose_table_and_degenerate_segment(gpu_ctx):
    """A one-row table: every pose is that row, so p' = p.  A table with a repeated time (inv_dt = 0):
    as the oracle."""
    rng = np.random.default_rng(3)
    counts = np.array([1500, 0, 7])
    n = int(counts.sum())
    rows = Q.f32(np.column_stack([rng.uniform(-90, 90, (n, 3)), rng.uniform(0, 1, n)]))
    t_ns = rng.integers(0, 100_000_000, n)
    times = np.array([1.0, 2.0, 3.0])
    b = gpu_ctx.batch(counts, with_time=True)
    b.upload_aos(rows)
    b.upload_time(t_ns)
    b.set_frame_times(times)
    gpu_ctx.set_trajectory([3.0], [[1.0e5, 2.0e6, 3.0]], [[0.1, -0.2, 2.5]])
    got = gpu_ctx.deskew(b, mode="pose_slerp", reference="end").download_aos()
    assert_scaled_close(got[:, :3], rows[:, :3], np.linalg.norm(rows[:, :3], axis=1), what="one-row table")
    tr = {"time": np.array([0.0, 1.0, 1.0, 1.05, 2.0, 4.0]),
          "position_gps": np.array([4e5, 5e6, 10.0]) + np.cumsum(rng.normal(0, 2.0, (6, 3)), axis=0),
          "orientation_imu": np.cumsum(rng.normal(0, 0.3, (6, 3)), axis=0)}
    _set_table(gpu_ctx, tr)
    t_ref = np.array([1.0, 0.5, 3.5])
    got = gpu_ctx.deskew(b, mode="pose_slerp", reference=t_ref).download_aos()
    off = np.concatenate([[0], np.cumsum(counts)])
    for f in (0, 2):
        s = slice(off[f], off[f + 1])
        ref = V.relative_oracle(rows[s, :3], t_ns[s], times[f], t_ref[f], tr)
        assert_scaled_close(got[s, :3], ref, V.relative_scale(rows[s, :3], t_ns[s], times[f], t_ref[f], tr),
                            what=f"degenerate segment frame {f}")


def test_pose_at(gpu_ctx):
    tr = dict(Q.pose_table("big"))
    tr["position_gps"] = tr["position_gps"] + V.SHIFT
    _set_table(gpu_ctx, tr)
    rng = np.random.default_rng(9)
    time = tr["time"]
    t = np.concatenate([time[[0, 1, 1234, len(time) - 1]], rng.uniform(time[0], time[-1], 300),
                        [time[0] - 5.0, time[-1] + 5.0, -1e9, 1e9]])
    Rg, pg = gpu_ctx.pose_at(t)
    Rw, pw = R.slerp_pose(time, tr["position_gps"], tr["orientation_imu"], t)
    assert Rg.shape == (len(t), 3, 3) and pg.shape == (len(t), 3)
    assert np.abs(Rg - Rw).max() <= 1e-13
    assert np.all(np.abs(pg - pw) <= 4 * np.spacing(np.abs(pw)))
    # at a pose sample the pose is that sample's
    assert np.abs(Rg[2] - R.euler_xyz_matrix(tr["orientation_imu"][1234])).max() <= 1e-13
    assert np.array_equal(pg[2], tr["position_gps"][1234])
    R1, p1 = gpu_ctx.pose_at(float(t[7]))
    assert np.array_equal(R1[0], Rg[7]) and np.array_equal(p1[0], pg[7])
    with pytest.raises(ValueError):
        gpu_ctx.pose_at([1.0, np.nan])


def test_time_spans(gpu_ctx):
    rng = np.random.default_rng(4)
    counts = np.array([3000, 0, 1, 1025])
    t = rng.integers(-2_000_000_000, 2_000_000_000, int(counts.sum())).astype(np.int32)
    b = gpu_ctx.batch(counts, with_time=True)
    b.upload_time(t)
    lo, hi = b.time_spans()
    off = np.concatenate([[0], np.cumsum(counts)])
    for f, n in enumerate(counts):
        if n:
            assert lo[f] == t[off[f]:off[f + 1]].min() and hi[f] == t[off[f]:off[f + 1]].max(), f
        else:
            assert lo[f] > hi[f]
    # after a per-point deskew carried t_ns into another batch, that batch's spans are its own
    gpu_ctx.set_trajectory([0.0, 10.0], np.zeros((2, 3)), np.zeros((2, 3)))
    b.set_frame_times(np.arange(4.0))
    o = gpu_ctx.deskew(b, gpu_ctx.batch(counts, with_time=True), mode="pose_slerp", reference="start")
    lo2, hi2 = o.time_spans()
    assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi)


def test_error_paths(mc, gpu_ctx):
    counts = np.array([10, 5])
    fresh = mc.Context(0)
    try:
        fb = fresh.batch(counts, with_time=True)
        fb.set_frame_times([0.0, 1.0])
        with pytest.raises(mc.McError, match="-4"):        # no trajectory
            fresh.deskew(fb, mode="pose_slerp", reference="start")
        with pytest.raises(mc.McError, match="-4"):
            fresh.pose_at([0.0])
        fb.close()
    finally:
        fresh.close()
    gpu_ctx.set_trajectory([0.0, 10.0], np.zeros((2, 3)), np.zeros((2, 3)))
    b = gpu_ctx.batch(counts, with_time=True)
    with pytest.raises(mc.McError, match="-4"):            # no frame times
        gpu_ctx.deskew(b, mode="pose_slerp", reference="start")
    with pytest.raises(mc.McError):
        gpu_ctx.deskew(b, mode="pose_slerp", reference="end")
    nt = gpu_ctx.batch(counts)
    nt.set_frame_times([0.0, 1.0])
    with pytest.raises(mc.McError, match="-4"):            # no t_ns column
        gpu_ctx.deskew(nt, mode="pose_slerp", reference="start")
    with pytest.raises(mc.McError, match="-4"):
        nt.time_spans()
    b.set_frame_times([0.0, 1.0])
    with pytest.raises(ValueError):                        # a NaN reference time
        gpu_ctx.deskew(b, mode="pose_slerp", reference=[0.5, np.nan])
    with pytest.raises(ValueError):
        gpu_ctx.deskew(b, mode="pose_slerp", reference=np.inf)
    with pytest.raises(ValueError):                        # one time per frame
        gpu_ctx.deskew(b, mode="pose_slerp", reference=[0.5, 0.6, 0.7])
    with pytest.raises(ValueError):
        gpu_ctx.deskew(b, mode="pose_slerp", reference="middle")
    for mode in ("frame", "imu"):                          # a reference with another mode
        with pytest.raises(ValueError):
            gpu_ctx.deskew(b, mode=mode, reference="start")
    with pytest.raises(ValueError):
        mc.runtime.deskew_points_f64(gpu_ctx, "imu", [1], np.zeros((1, 3)), [0], frame_start_ns=[0], t_ref=[0.0])
    with pytest.raises(ValueError):
        mc.runtime.deskew_points_f64(gpu_ctx, "pose_slerp", [1], np.zeros((1, 3)), [0], frame_times=[0.0], t_ref=[np.nan])
    # the batch still works after the refused calls
    out = gpu_ctx.deskew(b, mode="pose_slerp", reference="start").download_aos()
    assert out.shape == (15, 4)


def test_deskew_frames_reference(mc, gpu_ctx):
    """LiDARMotionSimulator.deskew_frames(reference=...) on float64 rows (mc_deskew_points_relative_f64)."""
    rng = np.random.default_rng(12)
    T = 300
    tr = {"time": np.linspace(0, 30, T), "position_gps": np.array([5e5, 5.4e6, 300.0]) + np.cumsum(rng.normal(0, 0.5, (T, 3)), axis=0),
          "orientation_imu": np.cumsum(rng.normal(0, 0.1, (T, 3)), axis=0)}
    counts = [700, 0, 3, 40_000]                               # the last frame takes the staged (DMA) path
    frames = [np.column_stack([rng.uniform(-90, 90, (n, 3)), rng.uniform(0, 1, n)]) for n in counts]
    t_ns = [rng.integers(-3_000_000_000, 6_000_000_000, n) for n in counts]      # beyond int32 ns
    times = np.array([0.5, 1.0, 2.0, 29.9])
    sim = mc.LiDARMotionSimulator(context=gpu_ctx)
    for reference in ("start", "end", 12.5, times + 0.25):
        out = sim.deskew_frames(frames, t_ns, tr, times, reference=reference)
        t_ref = (V.reference_times(times, t_ns, reference) if isinstance(reference, str)
                 else np.broadcast_to(np.asarray(reference, np.float64), (4,)))
        for f, n in enumerate(counts):
            assert out[f].shape == (n, 4)
            if n == 0:
                continue
            a = (frames[f][:, :3], t_ns[f], times[f], t_ref[f], tr)
            assert_scaled_close(out[f][:, :3], V.relative_oracle(*a), V.relative_scale(*a), what=f"{reference!r} frame {f}")
            assert np.array_equal(out[f][:, 3], frames[f][:, 3])
    with pytest.raises(ValueError):
        sim.deskew_frames(frames, t_ns, tr, times, reference="middle")
