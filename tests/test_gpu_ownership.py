"""Who frees device memory: every block a context, a batch or the voxel filter allocates is owned by a
DevBuf (csrc/devbuf.hpp) and counted by mc_device_memory_live, so "destroying the handle frees
everything" is an equality of two readings.  The blocks mc_device_alloc hands out (DeviceBuffer) are the
caller's and are not in the account."""
import ctypes
import gc

import numpy as np
import pytest

import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu

CFG = dict(range_max=90.0, range_min=0.5, fov_horizontal=70.4, fov_vertical=77.2, lidar_range_noise=0.0)


def live(m):
    b, k = m._lib.c_int64(-1), m._lib.c_int64(-1)
    m._lib.check(m._lib.load().mc_device_memory_live(ctypes.byref(b), ctypes.byref(k)), "device_memory_live")
    return b.value, k.value


def fresh_context(m):
    """A context of this test's own whose handle the test destroys itself (no finalizer)."""
    ctx = m.Context(0)
    ctx._fin.detach()
    return ctx


def destroy_only(m, ctx):
    m._lib.check(ctx.lib.mc_destroy(ctx.handle), "mc_destroy")


def table(n, seed):
    """n poses over 0.1 s per step, and n IMU samples over the same span"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) * 0.1
    pos = np.cumsum(rng.uniform(0.0, 0.3, (n, 3)), axis=0)
    rpy = np.cumsum(rng.uniform(-0.02, 0.02, (n, 3)), axis=0)
    ts = (t * 1e9).astype(np.int64)
    gyro = rng.uniform(-0.2, 0.2, (n, 3))
    return t, pos, rpy, ts, gyro


def cloud_rows(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    r = np.column_stack([rng.uniform(-spread, spread, (n, 3)), rng.uniform(0.0, 255.0, n)])
    return r.astype(np.float32).astype(np.float64)


def ray_count(m, ctx, F, n_rays, seed):
    rng = np.random.default_rng(seed)
    pos = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (F, 3)))
    R = np.ascontiguousarray(np.tile(np.eye(3), (F, 1, 1)))
    d = rng.normal(size=(n_rays, 3))
    dirs = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True))
    steps = np.ascontiguousarray(np.arange(1, 41) * 0.5)
    counts = np.zeros(F, np.int64)
    p, cd, ci = m._lib.ptr, m._lib.c_double, m._lib.c_int64
    m._lib.check(ctx.lib.mc_ray_count(ctx.handle, F, p(pos, cd), p(R, cd), n_rays, p(dirs, cd), len(steps), p(steps, cd),
                                      0.5, p(counts, ci)), "ray_count")
    return counts


def test_destroy_alone_frees_all_a_context_can_own():
    m = pkg()
    lib, p, cd, ci = m._lib.load(), m._lib.ptr, m._lib.c_double, m._lib.c_int64
    gc.collect()
    start = live(m)
    ctx = fresh_context(m)
    assert live(m) > start   # the launch-span pool of mc_create

    for n in (8, 16):        # the second upload outgrows the first
        t, pos, rpy, ts, gyro = table(n, n)
        ctx.set_trajectory(t, pos, rpy)
        ctx.set_imu(ts, gyro)

    counts = [300, 0, 5]
    N = sum(counts)
    rows = cloud_rows(N, 1)
    t_ns = np.random.default_rng(2).integers(0, 90_000_000, N).astype(np.int32)
    inp = ctx.batch(counts, with_time=True, with_pcd_len=True)
    out = ctx.batch(counts, with_time=True, with_pcd_len=True)
    plain = ctx.batch(counts, with_time=True)        # an output without its own text sums (mc_deskew_pcd's scratch)
    inp.upload_aos(rows)
    inp.upload_time(t_ns)
    inp.set_frame_times(np.array([0.2, 0.5, 0.9]))
    inp.set_frame_starts(np.array([200_000_000, 500_000_000, 900_000_000], np.int64))
    for mode in ("frame", "pose_slerp", "imu"):
        ctx.deskew(inp, out, mode=mode)
    ctx.deskew(inp, out, mode="pose_slerp", reference="start")
    ctx.deskew(inp, out, mode="pose_slerp", reference=np.array([0.25, 0.55, 0.85]))
    ctx.sync()

    t64 = t_ns.astype(np.int64)
    m.runtime.deskew_points_f64(ctx, "pose_slerp", counts, rows, t64, frame_times=[0.2, 0.5, 0.9])
    m.runtime.deskew_points_f64(ctx, "imu", counts, rows, t64, frame_start_ns=[200_000_000, 500_000_000, 900_000_000])

    rot, trans = np.array([0.1, -0.2, 0.3]), np.array([1.0, 2.0, 3.0])
    for n in (10, 1 << 15):   # pinned zero-copy scratch, then the device staging buffer
        pts = cloud_rows(n, 3)
        res = np.empty((n, 4))
        m._lib.check(lib.mc_transform_pointcloud_f64(ctx.handle, p(pts, cd), n, 4, p(rot, cd), p(trans, cd), p(res, cd)),
                     "transform_pointcloud")

    for E in (600, 5000):     # the larger scene outgrows the visibility words
        ctx.set_environment(cloud_rows(E, 4 + E, spread=30.0))
        ctx.scan([0.2, 0.5, 0.9], dict(CFG, points_per_frame=200)).close()

    objs = cloud_rows(300, 5, spread=8.0)
    oc = np.array([150, 150], np.int64)
    m._lib.check(lib.mc_set_ray_scene(ctx.handle, 2, p(oc, ci), p(objs, cd), 4), "set_ray_scene")
    for n_rays in (64, 512):  # the per-chunk keys grow with the rays
        ray_count(m, ctx, 2, n_rays, n_rays)

    m.codecs.encode_pcd_batch(out)
    m.codecs.encode_lvx_batch(out, [1, 2, 3], [0.2, 0.5, 0.9])
    m.codecs.deskew_pcd_frames(inp, plain, mode="pose_slerp")

    for n in (300, 5000):     # left unreleased: mc_destroy has to free it
        assert m.voxel_downsample(cloud_rows(n, 6), 0.5, context=ctx).n_voxels > 0

    for b in (inp, out, plain):
        b.close()
    gc.collect()              # batches this test dropped on the way
    assert live(m) > start
    destroy_only(m, ctx)
    assert live(m) == start


def test_batch_frees_its_relative_tables():
    m = pkg()
    ctx = fresh_context(m)
    t, pos, rpy, _, _ = table(12, 7)
    ctx.set_trajectory(t, pos, rpy)
    counts = [257, 3]

    def relative_pair():
        inp = ctx.batch(counts, with_time=True)
        out = ctx.batch(counts, with_time=True)
        inp.upload_aos(cloud_rows(sum(counts), 8))
        inp.upload_time(np.random.default_rng(9).integers(0, 300_000_000, sum(counts)).astype(np.int32))
        inp.set_frame_times(np.array([0.3, 0.6]))
        made = live(m)
        ctx.deskew(inp, out, mode="pose_slerp", reference="start")
        ctx.sync()
        assert live(m)[1] == made[1] + 5    # d_roff, d_relw, d_tref, d_refpose and the records
        inp.close()
        out.close()

    relative_pair()          # the context's own staging scratch is allocated by now
    gc.collect()
    before = live(m)
    relative_pair()
    assert live(m) == before
    destroy_only(m, ctx)


def test_voxel_state_is_per_context_and_dies_with_it():
    m = pkg()
    lib = m._lib.load()
    gc.collect()
    start = live(m)
    rows = cloud_rows(700, 10)
    a = fresh_context(m)
    assert m.voxel_downsample(rows, 0.5, context=a).n_voxels > 0
    destroy_only(m, a)
    assert live(m) == start
    # a new context, at A's address or not, has no build and no timed launches
    b = fresh_context(m)
    assert lib.mc_voxel_emit_f64(b.handle, None, None, None) == m._lib.MC_ERR_STATE
    ms = np.zeros(4)
    n = m._lib.c_int64(-1)
    m._lib.check(lib.mc_timing_read_voxel(b.handle, m._lib.ptr(ms, m._lib.c_double), ctypes.byref(n)), "timing_read_voxel")
    assert n.value == 0 and not ms.any()
    # release frees early, twice is fine, and the next build is a whole one
    idle = live(m)
    assert m.voxel_downsample(rows, 0.5, context=b).n_voxels > 0
    assert live(m) > idle
    m._lib.check(lib.mc_voxel_release(b.handle), "voxel_release")
    assert live(m) == idle
    assert lib.mc_voxel_emit_f64(b.handle, None, None, None) == m._lib.MC_ERR_STATE
    m._lib.check(lib.mc_voxel_release(b.handle), "voxel_release (again)")
    want = V.downsample(rows, 0.5)
    cloud = m.voxel_downsample(rows, 0.5, context=b)
    assert cloud.n_voxels == len(want["rows"])
    assert np.array_equal(cloud.keys(), want["keys"]) and np.array_equal(cloud.point_counts(), want["counts"])
    assert np.array_equal(cloud.rows().view(np.uint64), want["rows"].view(np.uint64))
    destroy_only(m, b)
    assert live(m) == start


def test_scan_ray_and_codec_state_is_per_context_and_dies_with_it():
    m = pkg()
    lib, check, p = m._lib.load(), m._lib.check, m._lib.ptr
    cd, ci, ci32 = m._lib.c_double, m._lib.c_int64, m._lib.c_int32
    scene = cloud_rows(600, 11, spread=30.0)
    objs, oc = cloud_rows(300, 12, spread=8.0), np.array([150, 150], np.int64)
    counts, rows = [300, 0, 5], cloud_rows(305, 13)
    t, pos, rpy, _, _ = table(12, 14)
    F_ray, n_rays = 2, 64

    def three(ctx):
        """a scan's columns, a ray count's counts and hits, a PCD encode's bytes"""
        ctx.set_trajectory(t, pos, rpy)
        ctx.set_environment(scene)
        sb = ctx.scan([0.2, 0.5, 0.9], dict(CFG, points_per_frame=200))
        scan = (np.array(sb.counts), sb.download_aos())
        sb.close()
        check(lib.mc_set_ray_scene(ctx.handle, 2, p(oc, ci), p(objs, cd), 4), "set_ray_scene")
        hit_counts = ray_count(m, ctx, F_ray, n_rays, 15)
        hits = np.full(3 * F_ray * n_rays, -7, np.int32)
        check(lib.mc_ray_hits(ctx.handle, p(hits, ci32)), "ray_hits")
        pb = ctx.batch(counts)
        pb.upload_aos(rows)
        pcd = m.codecs.encode_pcd_batch(pb)
        pb.close()
        return scan, hit_counts, hits, pcd

    gc.collect()
    start = live(m)
    a = fresh_context(m)
    a.timing(True)
    got_a = three(a)
    assert got_a[0][0].sum() > 0 and got_a[1].sum() > 0   # the scan saw points, rays hit
    destroy_only(m, a)       # its scan, ray and codec timing pairs were never read
    assert live(m) == start
    # a new context, at A's address or not, has no count of either scanner and no timed launches
    b = fresh_context(m)
    buf = b.device_buffer(64)
    assert lib.mc_scan_emit_f64(b.handle, None, buf.ptr, None) == m._lib.MC_ERR_STATE
    buf.close()
    r_inv = np.ascontiguousarray(np.tile(np.eye(3).ravel(), F_ray))
    assert lib.mc_ray_emit_f64(b.handle, p(r_inv, cd), None, p(np.zeros(5 * F_ray * n_rays), cd)) == m._lib.MC_ERR_STATE
    assert lib.mc_ray_hits(b.handle, p(np.zeros(3 * F_ray * n_rays, np.int32), ci32)) == m._lib.MC_ERR_STATE
    for name in ("scan", "ray", "codec"):
        ms, n = cd(-1.0), ci(-1)
        check(getattr(lib, f"mc_timing_read_{name}")(b.handle, ctypes.byref(ms), ctypes.byref(n)), f"timing_read_{name}")
        assert n.value == 0 and ms.value == 0.0, name
    got_b = three(b)
    assert np.array_equal(got_a[0][0], got_b[0][0])
    assert np.array_equal(got_a[0][1].view(np.uint64), got_b[0][1].view(np.uint64))
    assert np.array_equal(got_a[1], got_b[1]) and np.array_equal(got_a[2], got_b[2])
    assert got_a[3] == got_b[3]
    destroy_only(m, b)
    assert live(m) == start


def every_analysis(m, ctx, rows):
    """A build of ``rows`` at h = 0.5 and every analysis of it once, from rows and from a small batch, with nothing
    of the timing read and the cloud left live -> every result, arrays as their bytes."""
    cloud = m.voxel_downsample(rows, 0.5, context=ctx)
    src = rows[:200] + np.array([0.05, -0.03, 0.02, 0.0])
    normals = cloud.normals(1.0, max_nn=8, covariance=True)          # eight of more neighbours: the cap's launch too
    clusters = cloud.clusters(0.8, min_points=3)
    ground = cloud.segment_plane(0.3, num_iterations=64, seed=3)
    rest = ~ground.inliers
    assert ground.n_inliers >= 3 and rest.sum() >= 3 and clusters.n_clusters > 0 and normals.counts.max() == 8
    second = cloud.segment_plane(0.3, num_iterations=64, seed=4, refine=True, among=rest)
    picked = cloud.select(rest)
    selected = picked.download_aos()
    picked.close()
    batch = ctx.batch([40, 0, 25])
    batch.upload_aos(src[:65])
    near = (cloud.nearest(src[:, :3], 1.0), cloud.nearest(batch, 1.0, frame=2))
    reg = (cloud.register(src[:, :3], 1.0, max_iterations=3), cloud.register(batch, 1.0, max_iterations=3))
    batch.close()
    assert (near[0].ids >= 0).any() and reg[0].pairs >= 6 and reg[0].iterations >= 1
    out = [cloud.rows(), cloud.keys(), cloud.point_counts(), selected]
    for result in (normals, clusters, ground, second) + near + reg:
        out.extend(result)
    return [v.tobytes() if isinstance(v, np.ndarray) else v for v in out]


def test_the_analyses_scratch_and_unread_timing_die_with_the_state():
    """The filter's neighbour above, for what the four analyses keep in the voxel state: their scratch and the timing
    pairs of every phase, none of them read, go with mc_destroy alone and with mc_voxel_release."""
    m = pkg()
    lib = m._lib.load()
    rows = cloud_rows(700, 10, spread=4.0)
    gc.collect()
    start = live(m)
    # (a) destroy alone
    a = fresh_context(m)
    a.timing(True)
    first = every_analysis(m, a, rows)
    assert live(m) > start
    destroy_only(m, a)
    assert live(m) == start
    # (b) release: the level the context idles at once its own scratch exists
    b = fresh_context(m)
    b.timing(True)
    assert every_analysis(m, b, rows) == first
    m._lib.check(lib.mc_voxel_release(b.handle), "voxel_release")
    idle = live(m)
    m._lib.check(lib.mc_voxel_release(b.handle), "voxel_release (again)")          # (c)
    assert live(m) == idle
    for read in (b.read_timing_voxel, b.read_timing_normals, b.read_timing_clusters, b.read_timing_plane,
                 b.read_timing_register):                                            # (d)
        t = read()
        assert t.pop("regions") == 0 and len(t) >= 3 and not any(t.values()), (read.__name__, t)
    assert every_analysis(m, b, rows) == first                                       # (e)
    assert live(m) > idle
    t = b.read_timing_register()
    assert t["regions"] > 0 and t["solve_ms"] > 0.0
    m._lib.check(lib.mc_voxel_release(b.handle), "voxel_release")
    assert live(m) == idle
    destroy_only(m, b)
    assert live(m) == start
