"""The registration of a source against a voxel cloud on the device (VoxelCloud.nearest, VoxelCloud.register;
csrc/register.hpp) against the NumPy restatement of tests/registration.py: the nearest voxel and its squared distance
of every point, every row of the history (pairs, sum r^2, the step), the final pose, the status, the fitness and the
rmse are equal bit for bit, and a second call equals the first byte for byte.  The restatement takes the cloud's
normals as an input: the bits of VoxelCloud.normals(normals_radius, max_nn) of the same cloud, which the registration
computes for itself on the device and never downloads."""
import ctypes

import numpy as np
import pytest

import registration as G
from conftest import pkg

pytestmark = pytest.mark.gpu


def raw(r):
    parts = [r.transformation, r.history, np.float64([r.fitness, r.inlier_rmse]), np.int64([r.pairs, r.iterations]),
             np.frombuffer(r.status.encode(), np.uint8)]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def shapes_hold(r, near, n):
    return (r.transformation.shape == (4, 4) and r.transformation.dtype == np.float64 and r.history.shape == (r.iterations, 8)
            and r.history.dtype == np.float64 and isinstance(r.fitness, float) and isinstance(r.inlier_rmse, float)
            and isinstance(r.pairs, int) and isinstance(r.iterations, int) and r.status in G.STATUS
            and near.ids.shape == (n,) and near.ids.dtype == np.int32 and near.dist2.shape == (n,) and near.dist2.dtype == np.float64)


def cloud_of(m, ctx, c):
    cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
    assert np.array_equal(cloud.rows()[:, :3].view(np.uint64), c["cent"].view(np.uint64))
    return cloud


def check(cloud, c, want, src, frame=None, what=""):
    """nearest and register of src on the cloud against the restatement `want`, twice."""
    n = len(want["ids"][0])
    near = cloud.nearest(src, c["max_distance"], transform=c["init"], frame=frame)
    kw = dict(init=c["init"], max_iterations=c["max_iterations"], normals_radius=c["radius"], max_nn=c["max_nn"], frame=frame)
    got = cloud.register(src, c["max_distance"], **kw)
    print(f"{what}: {got.status} ({want['status']}) after {got.iterations} ({want['iterations']}), pairs {got.pairs} "
          f"({want['pairs']}) of {n}, ids differing {int((near.ids != want['ids'][0]).sum())}, history differing in "
          f"{int((G.bits(got.history) != G.bits(want['history'])).sum()) if got.history.shape == want['history'].shape else -1} words")
    assert shapes_hold(got, near, n), what
    assert np.array_equal(near.ids, want["ids"][0]), what
    assert np.array_equal(G.bits(near.dist2), G.bits(want["dist2"][0])), what
    for i in range(min(got.iterations, want["iterations"])):
        assert np.array_equal(G.bits(got.history[i]), G.bits(want["history"][i])), (what, i, got.history[i], want["history"][i])
    assert G.equal(got, want), (what, got.status, want["status"])
    again = cloud.nearest(src, c["max_distance"], transform=c["init"], frame=frame)
    assert again.ids.tobytes() == near.ids.tobytes() and again.dist2.tobytes() == near.dist2.tobytes(), what
    assert raw(cloud.register(src, c["max_distance"], **kw)) == raw(got), what
    return got, near


def want_of(cloud, c, name):
    nrm = cloud.normals(c["radius"], c["max_nn"])
    return G.expect_case(name, nrm.normals, nrm.counts)


@pytest.mark.parametrize("name", list(G.CASES))
def test_every_case_equals_the_restatement_twice(gpu_ctx, name):
    """Source sizes 1, 255, 256, 257 and 1281 (the tree's block edge and padded partials); windows of W = 1, 2 and 4;
    a tie, the lower cell key winning; a centroid at exactly max_distance taken, and not at the float64 below; windows
    that cross the key range's ends, queries in empty cells and at negative keys, a NaN, an infinity and two points
    beyond the key range among the source; a nearest voxel with fewer than three neighbours; five pairs; a source on
    one plane; the known answer, its history row by row, from the answer, and cut to one iteration."""
    m = pkg()
    c = G.case(name)
    cloud = cloud_of(m, gpu_ctx, c)
    got, near = check(cloud, c, want_of(cloud, c, name), c["src"], what=name)
    if name == "tie":
        assert near.ids.tolist() == G.TIE_WINNERS
    if name.startswith("radius edge"):
        assert near.ids.tolist() == ([-1, -1, -1, 0] if "below" in name else [0, 0, 0, 0])
    if name.startswith("window edges"):
        assert near.ids[-4:].tolist() == [-1] * 4 and np.isinf(near.dist2[-4:]).all() and near.ids[:8].tolist() == list(range(8))
    if name == "few neighbours":
        assert got.status == "too_few_pairs" and got.pairs == 5 and np.array_equal(got.transformation, np.eye(4))
    if name == "one plane":
        assert got.status == "singular" and np.array_equal(got.transformation, c["init"]) and got.iterations == 1
    if name == "known answer":
        assert got.status == "converged" and got.fitness == 1.0
        assert np.abs(got.transformation - G.KNOWN).max() <= 4 * 1.12e-16        # tests/test_registration_cpu.py's measurement
    if name == "known answer, one iteration":
        assert got.status == "max_iterations" and got.iterations == 1
    if name == "known answer from the answer":
        assert got.status == "converged" and got.iterations == 1


def test_a_third_tree_level(gpu_ctx):
    """65 537 source points: 512 first-level partials per sum, a second level of 2, the host's last level."""
    m = pkg()
    c = G.known_answer(65537, 2)
    c.update(G.corner())
    cloud = cloud_of(m, gpu_ctx, c)
    nrm = cloud.normals(c["radius"], c["max_nn"])
    want = G.register(G.with_normals(c, nrm.normals, nrm.counts), c["src"], c["max_distance"], max_iterations=2)
    got, _ = check(cloud, c, want, c["src"], what="65537 points")
    assert got.iterations == 2 and got.pairs == 65537


def test_batch_and_rows_and_one_frame(gpu_ctx):
    """The same float32 values as a Batch of frames of 400, 0 and 881 points and as float64 rows: the same bytes; then
    frame 0 and frame 2 alone, against the restatement of those rows."""
    m = pkg()
    ctx = gpu_ctx
    name = "slab 1281 from a pose"
    c = dict(G.case(name))
    src = c["src"].astype(np.float32).astype(np.float64)
    b = ctx.batch([400, 0, 881])
    b.upload_columns(*[src[:, k].astype(np.float32) for k in range(3)], np.zeros(len(src), np.float32))
    cloud = cloud_of(m, ctx, c)
    nrm = cloud.normals(c["radius"], c["max_nn"])
    given = G.with_normals(c, nrm.normals, nrm.counts)
    kw = dict(init=c["init"], max_iterations=c["max_iterations"])
    want = G.register(given, src, c["max_distance"], **kw)
    from_rows, _ = check(cloud, c, want, src, what="rows")
    from_batch, _ = check(cloud, c, want, b, what="batch")
    assert raw(from_rows) == raw(from_batch)
    for f, part in ((0, src[:400]), (2, src[400:])):
        check(cloud, c, G.register(given, part, c["max_distance"], **kw), b, frame=f, what=f"frame {f}")
    with pytest.raises(ValueError, match="empty"):
        cloud.nearest(b, c["max_distance"], frame=1)
    with pytest.raises(ValueError, match="frame"):
        cloud.register(b, c["max_distance"], frame=3)
    other = m.Context(0)
    with pytest.raises(ValueError, match="another context"):
        cloud.nearest(other.batch([4]), c["max_distance"])
    assert ctx.lib.mc_voxel_nearest_batch(ctx.handle, other.batch([4]).handle, -1, c["max_distance"], None, None, None) == m._lib.MC_ERR_INVALID


def test_state_lifetime_and_timing(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    name = "known answer"
    c = G.case(name)
    cloud = cloud_of(m, ctx, c)
    before = (cloud.rows().tobytes(), cloud.keys().tobytes(), cloud.point_counts().tobytes())
    plane = cloud.segment_plane(c["h"], 50, 1)
    want = want_of(cloud, c, name)
    ctx.read_timing_register()
    ctx.timing(True)
    try:
        got = cloud.register(c["src"], c["max_distance"])
    finally:
        ctx.timing(False)
    t = ctx.read_timing_register()
    assert G.equal(got, want)
    assert set(t) == {"normals_ms", "correspond_ms", "leaves_ms", "tree_ms", "solve_ms", "regions"}
    assert all(t[k] > 0 for k in ("normals_ms", "correspond_ms", "leaves_ms", "solve_ms")) and t["tree_ms"] == 0.0, t
    assert t["regions"] >= 1 + 3 * got.iterations
    assert ctx.read_timing_register() == {"normals_ms": 0.0, "correspond_ms": 0.0, "leaves_ms": 0.0, "tree_ms": 0.0,
                                          "solve_ms": 0.0, "regions": 0}
    # the cloud is what it was, and so is what the other calls give on it
    assert (cloud.rows().tobytes(), cloud.keys().tobytes(), cloud.point_counts().tobytes()) == before
    after = cloud.segment_plane(c["h"], 50, 1)
    assert after.model.tobytes() == plane.model.tobytes() and after.inliers.tobytes() == plane.inliers.tobytes()
    # the C entries' own refusals
    lib, h = ctx.lib, ctx.handle
    n = len(c["src"])
    rows = ctx.device_buffer(24 * n)
    rows.from_host(np.ascontiguousarray(c["src"]))
    ids, d2 = ctx.device_buffer(4 * n), ctx.device_buffer(8 * n)
    bad = np.eye(4)
    bad[0, 0] = 1.001
    P = lambda a: m._lib.ptr(a, ctypes.c_double)
    for args in ((rows.ptr, 3, n, 0.0, None), (rows.ptr, 3, n, float("nan"), None), (rows.ptr, 3, n, 4.5 * c["h"], None),
                 (rows.ptr, 2, n, 0.5, None), (rows.ptr, 3, 0, 0.5, None), (None, 3, n, 0.5, None), (rows.ptr, 3, n, 0.5, P(bad))):
        assert lib.mc_voxel_nearest_f64(h, *args, ids.ptr, d2.ptr) == m._lib.MC_ERR_INVALID, args
    assert lib.mc_voxel_nearest_f64(h, rows.ptr, 3, n, 0.5, None, None, d2.ptr) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_nearest_f64(h, rows.ptr, 3, n, 0.5, None, ids.ptr, d2.ptr) == m._lib.MC_OK
    assert np.array_equal(ids.to_host(np.int32, count=n), want["ids"][0])
    par = m._lib.RegisterParams(0.5, 0.5, 1e-6, 1e-6, (ctypes.c_double * 16)(*np.eye(4).reshape(-1)), 30, 30)
    T, hist, stats = np.zeros(16), np.zeros((30, 8)), np.zeros(4, np.int64)
    out = (P(T), P(hist), m._lib.ptr(stats, ctypes.c_int64))
    assert lib.mc_voxel_register_f64(h, rows.ptr, 3, n, ctypes.byref(par), *out) == m._lib.MC_OK
    assert stats.tolist() == [want["pairs"], want["iterations"], 0, n] and np.array_equal(G.bits(T.reshape(4, 4)), G.bits(want["transformation"]))
    for field, value in (("max_iterations", 0), ("max_iterations", 2 ** 16 + 1), ("max_nn", 2), ("normals_radius", 0.0),
                         ("normals_radius", 1.5), ("max_distance", -1.0), ("tol_rotation", -1.0), ("tol_translation", float("nan"))):
        q = m._lib.RegisterParams.from_buffer_copy(par)
        setattr(q, field, value)
        assert lib.mc_voxel_register_f64(h, rows.ptr, 3, n, ctypes.byref(q), *out) == m._lib.MC_ERR_INVALID, field
        assert stats.tolist() == [0, 0, -1, 0] or stats.tolist() == [0, 0, -1, n]
    assert lib.mc_voxel_register_f64(h, rows.ptr, 3, n, None, *out) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_register_f64(h, rows.ptr, 3, n, ctypes.byref(par), None, out[1], out[2]) == m._lib.MC_ERR_INVALID
    # an empty cloud: nobody has a nearest voxel
    none = m.voxel_downsample(np.zeros((0, 4)), 0.25, context=ctx)
    near = none.nearest(c["src"][:300], 0.5)
    assert (near.ids == -1).all() and np.isinf(near.dist2).all()
    r = none.register(c["src"][:300], 0.5)
    assert r.status == "too_few_pairs" and r.pairs == 0 and r.iterations == 1 and r.fitness == 0.0 and r.inlier_rmse == 0.0
    # a later build on the context ends the cloud; so does close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.nearest(c["src"], 0.5)
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.register(c["src"], 0.5)
    none.close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        none.register(c["src"], 0.5)
    assert lib.mc_voxel_nearest_f64(h, rows.ptr, 3, n, 0.5, None, ids.ptr, d2.ptr) == m._lib.MC_ERR_STATE
    assert lib.mc_voxel_register_f64(h, rows.ptr, 3, n, ctypes.byref(par), *out) == m._lib.MC_ERR_STATE
