"""The voxel-grid filter on the device, bit for bit against the NumPy restatement of tests/voxel.py: the
order of the voxels, their keys, counts and float64 rows, and the float32 batch.  Every case goes
through both sources (a Batch of float32 columns, float64 rows)."""
import ctypes

import numpy as np
import pytest

import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_cloud(cloud, want, what):
    assert cloud.n_voxels == len(want["rows"]), what
    assert np.array_equal(cloud.keys(), want["keys"]), what
    assert np.array_equal(cloud.point_counts(), want["counts"]), what
    assert np.array_equal(bits(cloud.rows()), bits(want["rows"])), what
    b = cloud.batch()
    assert b.n_frames == 1 and b.n_points == cloud.n_voxels and not b.with_time
    got = np.stack(b.download_columns(), axis=1) if cloud.n_voxels else np.zeros((0, 4), np.float32)
    assert np.array_equal(bits(got), bits(want["f32"])), what
    return b


def both_sources(ctx, counts, rows, h, origin=(0.0, 0.0, 0.0), what="", want=None):
    """rows: (N, 4) float64 holding float32 values, frame-major; want: V.downsample(rows, h, origin) where
    the caller has it already.  -> (restatement, last cloud)"""
    m = pkg()
    rows = np.ascontiguousarray(rows, np.float64)
    assert np.array_equal(rows, rows.astype(np.float32).astype(np.float64))
    if want is None:
        want = V.downsample(rows, h, origin)
    b = ctx.batch(counts)
    b.upload_columns(*[rows[:, c].astype(np.float32) for c in range(4)])
    check_cloud(ctx.voxel_downsample(b, h, origin), want, f"{what} (batch)")
    cloud = m.voxel_downsample(rows, h, origin, context=ctx)
    check_cloud(cloud, want, f"{what} (rows)")
    return want, cloud


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def test_padding_slots_are_not_points(gpu_ctx):
    """Frames of 1, 255, 256, 257, 0 and 1000 points, all inside voxel (0, 0, 0): a padding slot counted
    by mistake (whatever it holds) changes the count, a zero there lands in this very voxel."""
    counts = [1, 255, 256, 257, 0, 1000]
    rng = np.random.default_rng(1)
    rows = f32(rng.uniform(0.05, 0.95, (sum(counts), 4)))
    want, _ = both_sources(gpu_ctx, counts, rows, 1.0, what="padding")
    assert want["counts"].tolist() == [sum(counts)] and want["keys"].tolist() == [[0, 0, 0]]
    # and spread over voxels, frames ending inside blocks
    rows[:, :3] = f32(rng.uniform(-3.0, 3.0, (sum(counts), 3)))
    both_sources(gpu_ctx, counts, rows, 0.5, what="padding, many voxels")


def test_contention_in_one_voxel(gpu_ctx):
    rng = np.random.default_rng(2)
    rows = f32(np.column_stack([rng.uniform(10.01, 10.19, (4096, 3)) - [0, 20, 0], rng.uniform(0, 255, 4096)]))
    want, _ = both_sources(gpu_ctx, [4096], rows, 0.2, what="contention")
    assert want["counts"].tolist() == [4096]


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_every_point_its_own_voxel(gpu_ctx, n):
    """The table at its fullest on both sides of a capacity step (4096 slots for 2048 points, 8192 for 2049)."""
    rng = np.random.default_rng(n)
    i = rng.permutation(n)
    keys = np.stack([i % 13 - 6, (i // 13) % 17 - 8, i // 221 - 4], axis=1)
    rows = f32(np.column_stack([(keys + rng.uniform(0.1, 0.9, (n, 3))) * 0.25, rng.uniform(0, 1, n)]))
    want, _ = both_sources(gpu_ctx, [n], rows, 0.25, what=f"own voxel, n = {n}")
    assert len(want["rows"]) == n and np.array_equal(want["keys"], keys)


def test_many_workgroups_with_duplicates_across_frames(gpu_ctx):
    """70 001 points over 7 frames (35 chunks of the rank scan), about 9 000 voxels whose points are
    interleaved across the frames."""
    counts = [10000, 10001, 9999, 10003, 9998, 10000, 10000]
    n = sum(counts)
    assert n == 70001
    rng = np.random.default_rng(3)
    centre = rng.integers(-40, 40, (9000, 3))
    pick = rng.integers(0, 9000, n)
    rows = f32(np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (n, 3))) * 0.2, rng.uniform(0, 1, n)]))
    want, _ = both_sources(gpu_ctx, counts, rows, 0.2, what="70 001 points")
    assert 5000 < len(want["rows"]) <= 9000 and want["counts"].max() >= 8


@pytest.mark.parametrize("grid", range(len(V.GRIDS)))
def test_boundary_and_range_values(gpu_ctx, grid):
    m = pkg()
    h, origin = V.GRIDS[grid]
    acc32, _ = V.edge_rows(h, origin, np.float32)
    both_sources(gpu_ctx, [len(acc32)], acc32, h, origin, what=f"edges float32 {h} {origin}")
    acc64, _ = V.edge_rows(h, origin, np.float64)     # values only float64 rows can hold
    check_cloud(m.voxel_downsample(acc64, h, origin, context=gpu_ctx), V.downsample(acc64, h, origin), "edges float64")


def test_refusals_name_the_lowest_point_and_leave_nothing(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    counts = [300, 0, 700, 1100]
    rng = np.random.default_rng(4)
    good = f32(rng.uniform(-5, 5, (sum(counts), 4)))
    _, ref = V.edge_rows(0.1, (0.0, 0.0, 0.0), np.float32)
    ok_cloud = m.voxel_downsample(good, 0.1, context=ctx)
    for k, bad_row in enumerate(ref):
        rows = good.copy()
        at = sorted(({300 + (37 * k) % 700} if k % 2 == 0 else set()) | {1000 + (91 * k) % 1100, 2099})   # frames 2, 3
        rows[at] = bad_row
        with pytest.raises(V.Refused) as e:
            V.downsample(rows, 0.1)
        assert e.value.index == at[0]
        b = ctx.batch(counts)
        b.upload_columns(*[rows[:, c].astype(np.float32) for c in range(4)])
        frame, index = (2, at[0] - 300) if at[0] < 1000 else (3, at[0] - 1000)
        with pytest.raises(ValueError, match=rf"frame {frame}, point {index} "):
            ctx.voxel_downsample(b, 0.1)
        with pytest.raises(ValueError, match=rf"row {at[0]} "):
            m.voxel_downsample(rows, 0.1, context=ctx)
        if k % 7 == 0:   # nothing is left to emit: the library says so itself, and the earlier cloud is void
            buf = ctx.device_buffer(64)
            assert ctx.lib.mc_voxel_emit_f64(ctx.handle, buf.ptr, None, None) == m._lib.MC_ERR_STATE
            out = ctx.batch([1])
            assert ctx.lib.mc_voxel_emit_batch(ctx.handle, out.handle) == m._lib.MC_ERR_STATE
            with pytest.raises(ValueError):
                ok_cloud.rows()
    # a wrong-sized out batch, after a good build
    cloud = m.voxel_downsample(good, 0.1, context=ctx)
    for shape in ([cloud.n_voxels + 1], [cloud.n_voxels - 1], [cloud.n_voxels, 0]):
        assert ctx.lib.mc_voxel_emit_batch(ctx.handle, ctx.batch(shape).handle) == m._lib.MC_ERR_INVALID
    o = np.zeros(3)
    n = ctypes.c_int64()
    for h in (0.0, -1.0, float("nan"), float("inf")):
        assert ctx.lib.mc_voxel_build_f64(ctx.handle, None, 4, 0, h, m._lib.ptr(o, ctypes.c_double), ctypes.byref(n),
                                          None) == m._lib.MC_ERR_INVALID
    assert ctx.lib.mc_voxel_build_f64(ctx.handle, None, 3, 0, 0.1, m._lib.ptr(o, ctypes.c_double), ctypes.byref(n),
                                      None) == m._lib.MC_ERR_INVALID
    empty = m.voxel_downsample(np.zeros((0, 4)), 0.1, context=ctx)
    assert empty.n_voxels == 0 and empty.rows().shape == (0, 4) and empty.batch().n_points == 0


def test_repeatable_bit_for_bit_and_out_of_the_codec(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    counts = [5000, 3000, 4001]
    rng = np.random.default_rng(5)
    rows = f32(np.column_stack([rng.normal(0, 3, (sum(counts), 3)), rng.uniform(0, 1, sum(counts))]))
    b = ctx.batch(counts)
    b.upload_columns(*[rows[:, c].astype(np.float32) for c in range(4)])
    want = V.downsample(rows, 0.3, (0.1, -0.2, 0.05))
    seen = []
    for _ in range(2):
        cloud = ctx.voxel_downsample(b, 0.3, (0.1, -0.2, 0.05))
        for _ in range(2):   # a second emit of the same build
            seen.append((cloud.rows(), cloud.point_counts(), cloud.keys(), np.stack(cloud.batch().download_columns(), 1)))
    for s in seen:
        assert np.array_equal(bits(s[0]), bits(want["rows"])) and np.array_equal(s[1], want["counts"])
        assert np.array_equal(s[2], want["keys"]) and np.array_equal(bits(s[3]), bits(want["f32"]))
    # out of the codec: the batch through the PCD writer = the restatement's float32 rows, "%.6f"
    out = cloud.batch(with_pcd_len=True)
    assert not out.pcd_len_current()
    body = "".join("%.6f %.6f %.6f %.6f\n" % tuple(r) for r in want["f32"].astype(np.float64).tolist())
    assert m.codecs.encode_pcd_batch(out) == [m.codecs.pcd_header(len(want["f32"])) + body.encode("ascii")]
    cloud.close()
    with pytest.raises(ValueError):
        cloud.rows()


def test_no_leak_into_the_deskew(gpu_ctx):
    """The same deskew before and after a voxel call on the same context: identical output."""
    m = pkg()
    ctx = gpu_ctx
    sim = m.LiDARMotionSimulator({"duration": 10.0, "trajectory_type": "figure_eight"}, context=ctx)
    tr = sim.add_sensor_noise(sim.generate_trajectory())
    counts = [3000, 17, 2500, 0, 4096]
    b = ctx.batch(counts, with_time=True)
    b.synth(seed=3, frame_id_base=1000)
    b.set_frame_times(sim.lidar_times()[:len(counts)])
    ctx.set_trajectory(tr["time"], tr["position_gps"], tr["orientation_imu"])
    before = ctx.deskew(b, mode="pose_slerp")
    a0 = before.download_aos()
    cloud = ctx.voxel_downsample(before, 0.5)
    assert np.array_equal(bits(cloud.rows()), bits(V.downsample(a0, 0.5)["rows"]))
    assert np.array_equal(bits(before.download_aos()), bits(a0))        # the source is untouched
    a1 = ctx.deskew(b, mode="pose_slerp").download_aos()
    assert np.array_equal(bits(a1), bits(a0))
