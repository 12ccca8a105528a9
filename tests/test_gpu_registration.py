"""The registration of a source against a voxel cloud on the device (VoxelCloud.nearest, VoxelCloud.register;
csrc/register.hpp) against the NumPy restatement of tests/registration.py: the nearest voxel and its squared distance
of every point, every row of the history (pairs, sum r^2, the step), the final pose, the status, the fitness and the
rmse are equal bit for bit, and a second call equals the first byte for byte.  The restatement takes the cloud's
normals as an input: the bits of VoxelCloud.normals(normals_radius, max_nn) of the same cloud, which the registration
computes for itself on the device and never downloads."""
import ctypes

import numpy as np
import pytest

import clusters as C
import normals as N
import registration as G
import voxel as V
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


def grid_cloud(m, ctx, c, src=None):
    """The build of a grid case on its own h and origin (src: a Batch of the same values) and its precondition: the
    keys and the bits of the rows are the restatement's."""
    cloud = m.voxel_downsample(c["rows"] if src is None else src, c["h"], c["origin"], context=ctx)
    assert np.array_equal(cloud.keys(), c["keys"])
    assert np.array_equal(cloud.rows().view(np.uint64), c["vox"]["rows"].view(np.uint64))
    return cloud


@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_grids_off_the_default_origin(gpu_ctx, grid):
    """The 257-point slab and 1281 scattered source points on every grid of V.ORIGIN_GRIDS (a UTM-scale origin with
    cloud and source there; an origin that is no multiple of h; far keys whose o + k h cancels; the same on
    h = 7.3), at W = 1, 2 and 4, from the identity and from G.NEARBY, for three iterations.  The restatement's
    nearest walks every cell of the window; the device leaves out what RegSkip says cannot win, from cell faces
    o + k h: here the o terms are not zero."""
    m = pkg()
    cloud = None
    for rel, init in G.GRID_RUNS:
        c = G.grid_case(grid, rel, init)
        cloud = grid_cloud(m, gpu_ctx, c) if cloud is None else cloud
        nrm = cloud.normals(c["radius"], c["max_nn"])
        want = G.grid_expect(grid, rel, init, nrm.normals, nrm.counts)
        got, near = check(cloud, c, want, c["src"], what=f"{grid}, {rel} h, {init}")
        assert (near.ids >= 0).sum() >= 200 and want["history"][0, 0] >= G.MIN_PAIRS          # the source is on the cloud


@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_the_radius_edge_on_every_grid(gpu_ctx, grid):
    """G.radius_edges: 64 queries whose nearest centroid is 0.3 h to 3.5 h away; max_distance the smallest float64
    whose square reaches that centroid's d2, where the restatement and the device must both take it, and the float64
    below, where neither may.  None is left out."""
    m = pkg()
    c = G.grid_case(grid)
    cloud = grid_cloud(m, gpu_ctx, c)
    edges = G.radius_edges(grid)
    assert len(edges) == G.EDGE_QUERIES == 64
    for i, e in enumerate(edges):
        assert e["at"] / c["h"] <= 3.5 < 4
        assert e["want_at"][0][0] >= 0, (grid, i)
        for md, (ids, d2) in ((e["at"], e["want_at"]), (e["under"], e["want_under"])):
            near = cloud.nearest(e["q"], md)
            assert np.array_equal(near.ids, ids), (grid, i, md, near.ids, ids)
            assert np.array_equal(G.bits(near.dist2), G.bits(d2)), (grid, i, md, near.dist2, d2)
            again = cloud.nearest(e["q"], md)
            assert again.ids.tobytes() == near.ids.tobytes() and again.dist2.tobytes() == near.dist2.tobytes()
        assert cloud.nearest(e["q"], e["at"]).ids[0] >= 0


@pytest.mark.parametrize("grid", [g for g in V.ORIGIN_GRIDS if V.ORIGIN_GRIDS[g]["batch"]])
def test_batch_and_rows_on_a_grid(gpu_ctx, grid):
    """Where float32 can hold the case: the cloud from a Batch and from float64 rows of the same float32 values, the
    source as a Batch of frames of 400, 0 and 881 points and as rows: the restatement's result and the same bytes in
    all four."""
    m = pkg()
    ctx = gpu_ctx
    c = G.grid_case(grid, 2.0, "nearby", float32=True)
    cb = ctx.batch([100, 0, len(c["rows"]) - 100])
    cb.upload_columns(*[c["rows"][:, k].astype(np.float32) for k in range(4)])
    sb = ctx.batch([400, 0, 881])
    sb.upload_columns(*[c["src"][:, k].astype(np.float32) for k in range(3)], np.zeros(len(c["src"]), np.float32))
    seen = []
    for cloud_src in (None, cb):
        cloud = grid_cloud(m, ctx, c, cloud_src)
        nrm = cloud.normals(c["radius"], c["max_nn"])
        want = G.grid_expect(grid, 2.0, "nearby", nrm.normals, nrm.counts, float32=True)
        for src in (c["src"], sb):
            got, near = check(cloud, c, want, src, what=f"{grid}: cloud {'batch' if cloud_src else 'rows'}, source "
                                                        f"{'rows' if src is c['src'] else 'batch'}")
            seen.append(raw(got) + near.ids.tobytes() + near.dist2.tobytes())
    assert len(set(seen)) == 1


def exact_rows(n, seed):
    """N.slab's layer of h = 0.5 with every coordinate rounded to a multiple of 2^-8 (the points keep 0.05 h from
    their cells' faces, the rounding moves them by 2^-9): one point per voxel, every centroid its point exactly."""
    rows = N.slab(n, seed, 0.5)[0]
    rows[:, :3] = np.rint(rows[:, :3] * 256.0) / 256.0
    return rows


def test_two_exact_builds_agree_across_origins(gpu_ctx):
    """Without a restatement: h = 0.5 and coordinates that are multiples of 2^-8, once on the default grid and once
    moved by (64, -32, 8) onto a grid of that origin.  v - o, the fixed-point fractions, o + (k + s) h, every
    difference of two centroids and every product of two differences are exact in both, so the two builds must agree
    on the keys, the cluster labels and densities, the normals' counts and covariances, the unrefined plane's score,
    iteration, samples and inlier mask (its offsets s = n . c + d are exact, so s * s rounds alike), the refit's
    covariance, and the nearest ids and the bits of d2 of sources moved alike."""
    m = pkg()
    ctx = gpu_ctx
    h, shift = 0.5, np.array([64.0, -32.0, 8.0])
    rows = exact_rows(257, 257)
    src = np.rint(G.slab_source(1281, 1281, h) * 256.0) / 256.0
    seen = []
    for o in (np.zeros(3), shift):
        moved = rows.copy()
        moved[:, :3] += o
        cloud = m.voxel_downsample(moved, h, tuple(o), context=ctx)
        assert cloud.n_voxels == 257 and np.array_equal(cloud.rows()[:, :3], moved[:, :3])
        nrm = cloud.normals(2 * h, covariance=True)
        parts = [cloud.keys(), nrm.counts, nrm.covariance]
        for min_points, weighted in C.GRID_RUNS:
            cl = cloud.clusters(2 * h, min_points, weighted)
            parts += [cl.labels, cl.density]
        plain = cloud.segment_plane(h, 64, 257, False)
        refit = cloud.segment_plane(h, 64, 257, True)
        assert plain.score >= 3
        parts += [np.int64([plain.score, plain.iteration, plain.n_inliers]), plain.samples, plain.inliers,
                  np.int64([refit.score, refit.iteration]), refit.samples, refit.covariance]
        for rel in (0.9, 2.0, 4.0):
            near = cloud.nearest(src + o, rel * h)
            assert (near.ids >= 0).sum() >= 200
            parts += [near.ids, near.dist2]
        seen.append([np.ascontiguousarray(a).tobytes() for a in parts])
    differing = [i for i, (a, b) in enumerate(zip(*seen)) if a != b]
    assert not differing, differing


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
