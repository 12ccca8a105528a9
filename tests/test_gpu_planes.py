"""The plane segmentation of a voxel cloud and the selection of a subset into a batch on the device
(VoxelCloud.segment_plane, VoxelCloud.select; csrc/plane.hpp) against the NumPy restatement of tests/planes.py.
Scores, winner, samples, masks, the unrefined model and the refit's covariance are equal bit for bit; the refit's
normal passes the eigenvector criterion of tests/normals.py, is of unit length and signed by the rule, its d^ is
recomputed from it bit for bit; and a second call equals the first byte for byte.

The dyadic edge runs at two thresholds.  At t = 2^-4 the voxel at exactly t is an inlier and the voxel at the next
centroid the filter can hold above it (t + h 2^-32) is not.  A centroid at the next float64 above t cannot come out
of the filter, whose fixed point is h 2^-32; so the second run lowers the threshold to the float64 below t, and the
voxel at t — now at the next float64 above the threshold — is not an inlier."""
import ctypes

import numpy as np
import pytest

import clusters as C
import normals as N
import planes as P
import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def raw(r):
    parts = [r.model, r.inliers, np.int64([r.n_inliers, r.score, r.iteration, r.refined]), r.samples]
    if r.covariance is not None:
        parts.append(r.covariance)
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def shapes_hold(r, M):
    return (r.model.shape == (4,) and r.model.dtype == np.float64 and r.inliers.shape == (M,) and r.inliers.dtype == np.bool_
            and r.samples.shape == (3,) and r.samples.dtype == np.int32 and isinstance(r.refined, bool)
            and all(isinstance(v, int) for v in (r.n_inliers, r.score, r.iteration))
            and ((r.covariance is None) if not r.refined else (r.covariance.shape == (6,) and r.covariance.dtype == np.float64)))


def cloud_of(m, ctx, name):
    c = P.case(name)
    cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
    assert np.array_equal(cloud.rows()[:, :3].view(np.uint64), c["cent"].view(np.uint64))
    return c, cloud


def columns(batch):
    return np.stack(batch.download_columns(), axis=1) if batch.n_points else np.zeros((0, 4), np.float32)


@pytest.mark.parametrize("name", list(P.CASES))
def test_every_cloud_equals_the_restatement_twice(gpu_ctx, name):
    """The slabs: 3 voxels (one hypothesis possible), 255 / 256 / 257 around one workgroup and one tree block, 1281
    (six workgroup partials padded to eight); two equal planes: the tie goes to the lower k; collinear: no valid
    hypothesis, iteration -1; the dyadic edge (module docstring); ground + wall: the larger plane first."""
    m = pkg()
    c, cloud = cloud_of(m, gpu_ctx, name)
    for t in P.thresholds(name):
        for refine in (False, True):
            want = P.expect(name, refine, t)
            got = cloud.segment_plane(t, c["K"], c["seed"], refine)
            print(f"{name}: t {t!r} refine {refine}: iteration {got.iteration} ({want['iteration']}), score {got.score} "
                  f"({want['score']}), inliers {got.n_inliers} ({want['n_inliers']}), masks differing "
                  f"{int((got.inliers != want['inliers']).sum())}, model {got.model.tolist()} ({want['model'].tolist()})")
            assert shapes_hold(got, cloud.n_voxels)
            assert P.equal(got, want, refine), (name, t, refine)
            assert got.n_inliers == int(got.inliers.sum())
            assert raw(cloud.segment_plane(t, c["K"], c["seed"], refine)) == raw(got), (name, t, refine)


def test_one_more_hypothesis_than_a_score_chunk(gpu_ctx):
    """K = the library's score chunk + 1: a second launch of the score phase with a single hypothesis."""
    m = pkg()
    K = m.voxel.plane_score_chunk() + 1
    c, cloud = cloud_of(m, gpu_ctx, "slab 257")
    for refine in (False, True):
        want = P.expect("slab 257", refine, K=K)
        got = cloud.segment_plane(c["t"], K, c["seed"], refine)
        assert P.equal(got, want, refine)
    # a single hypothesis: the first of the table
    one = cloud.segment_plane(c["t"], 1, c["seed"], False)
    assert one.iteration == 0 and one.score == P.expect("slab 257", False, K=K)["scores"][0]


def test_batch_and_rows_give_the_same_bytes(gpu_ctx):
    """The same cloud built from a Batch and from float64 rows (values a batch can hold)."""
    m = pkg()
    ctx = gpu_ctx
    c = P.case("slab 1281")
    rows = c["rows"].astype(np.float32).astype(np.float64)
    b = ctx.batch([400, 0, 881])
    b.upload_columns(*[rows[:, k].astype(np.float32) for k in range(4)])
    seen = []
    for src in (rows, b):
        cloud = m.voxel_downsample(src, c["h"], context=ctx)
        assert cloud.n_voxels == 1281
        cent = cloud.rows()[:, :3]
        for refine in (False, True):
            got = cloud.segment_plane(c["t"], c["K"], c["seed"], refine)
            assert P.equal(got, dict(P.ransac(cent, c["t"], c["K"], c["seed"], refine), cent=cent), refine)
            seen.append(raw(got))
        seen.append(columns(cloud.select(got.inliers)).tobytes())
    assert seen[:3] == seen[3:]


def test_select(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    c, cloud = cloud_of(m, ctx, "slab 1281")
    M = cloud.n_voxels
    whole = columns(cloud.batch())
    assert np.array_equal(whole.view(np.uint32), c["vox"]["f32"].view(np.uint32))
    everything = cloud.select(np.ones(M, bool))
    assert everything.n_points == M and columns(everything).tobytes() == whole.tobytes()
    nothing = cloud.select(np.zeros(M, bool))
    assert nothing.n_points == 0 and nothing.n_frames == 1
    rng = np.random.default_rng(1281)
    for count in (255, 256, 257, 1, 1280):
        mask = np.zeros(M, bool)
        mask[rng.permutation(M)[:count]] = True
        got = cloud.select(mask)
        assert got.n_points == count and got.n_frames == 1
        assert columns(got).tobytes() == whole[mask].tobytes(), count
    # the last voxels alone, and a mask of one workgroup's voxels
    for mask in (np.arange(M) >= M - 3, (np.arange(M) >= 256) & (np.arange(M) < 512), np.arange(M) % 2 == 1):
        assert columns(cloud.select(mask)).tobytes() == whole[mask].tobytes()
    # the text of a selection is the text of the same rows uploaded by hand
    mask = np.arange(M) % 3 == 0
    sel = cloud.select(mask, with_pcd_len=True)
    hand = ctx.batch([int(mask.sum())], with_pcd_len=True)
    hand.upload_columns(*[np.ascontiguousarray(whole[mask][:, k]) for k in range(4)])
    assert m.codecs.encode_pcd_batch(sel) == m.codecs.encode_pcd_batch(hand)
    assert m.codecs.encode_pcd_batch(cloud.select(mask)) == m.codecs.encode_pcd_batch(hand)
    # a count mismatch at the C entry
    lib, h = ctx.lib, ctx.handle
    buf = ctx.device_buffer(M)
    buf.from_host(mask.view(np.uint8))
    for n in (int(mask.sum()) - 1, int(mask.sum()) + 1, 0, M):
        assert lib.mc_voxel_emit_selected(h, buf.ptr, ctx.batch([n]).handle) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_emit_selected(h, buf.ptr, ctx.batch([3, int(mask.sum()) - 3]).handle) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_emit_selected(h, None, ctx.batch([int(mask.sum())]).handle) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_emit_selected(h, buf.ptr, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_emit_selected(h, buf.ptr, ctx.batch([int(mask.sum())]).handle) == m._lib.MC_OK
    # a cloud of fewer voxels than one block, and the empty cloud
    c3, cloud3 = cloud_of(m, ctx, "slab 3")
    assert columns(cloud3.select(np.array([True, False, True]))).tobytes() == c3["vox"]["f32"][[0, 2]].tobytes()
    empty = m.voxel_downsample(np.zeros((0, 4)), 0.1, context=ctx)
    assert empty.select(np.zeros(0, bool)).n_points == 0


def large_runs():
    """(case, with among) of P.LARGE: the smallest size has no 257th workgroup count, so no candidates run."""
    return [(name, among) for name in P.LARGE for among in (False, True) if among is False or name != "slab 32769"]


@pytest.mark.parametrize("name,with_among", large_runs())
def test_sizes_where_the_code_changes_shape(gpu_ctx, name, with_among):
    """M = 32 769: the smallest cloud whose refit has a second tree level (65 536 leaves, one k_pl_tree<9> workgroup,
    half the first level padding).  M = 65 537: 131 072 leaves, two second-level workgroups and two partials for the
    host; and the first M with a 257th workgroup count in compact()'s scan, which the run among two voxels of every
    three takes.  M = 2048 * 1024 + 1025: 2 050 tiles on the score kernel's 2 048 workgroups, so workgroup 0 walks a
    full second tile and workgroup 1 a ragged one of one voxel, with and without candidates (K = 8: the restatement
    is the slow side).  Without a refit the score (the tiled kernel's) is the mask kernel's count, which has no tile
    loop; at the largest size the restatement's winner leads by more than a tile, so a wrong tile cannot hide
    behind a tie.  A third tree level on the device needs more than 8 388 608 voxels: left out, the restatement of
    such a cloud takes minutes."""
    m = pkg()
    c, cloud = cloud_of(m, gpu_ctx, name)
    M = cloud.n_voxels
    assert M == len(c["rows"]) == int(name.split()[1])
    among = P.among_of(M) if with_among else None
    key = "among" if with_among else None
    # with candidates the largest size runs once, refined: compact, the tiled score and the tree in one call
    for refine in ((True,) if with_among and M == P.TWO_TURNS else (False, True)):
        want = P.expect(name, refine, among=among, key=key)
        got = cloud.segment_plane(c["t"], c["K"], c["seed"], refine, among=among)
        top = np.sort(want["scores"])[-2:]
        print(f"{name}: among {with_among} refine {refine}: iteration {got.iteration} ({want['iteration']}), score {got.score} "
              f"({want['score']}), inliers {got.n_inliers} ({want['n_inliers']}), masks differing "
              f"{int((got.inliers != want['inliers']).sum())}; restatement scores {want['scores'].tolist()}")
        if M == P.TWO_TURNS:
            assert top[1] - top[0] > P.TILE, top
        assert shapes_hold(got, M)
        assert P.equal(got, want, refine), (name, with_among, refine)
        assert got.n_inliers == int(got.inliers.sum())
        if not refine:
            assert got.score == got.n_inliers == int(got.inliers.sum())
        assert raw(cloud.segment_plane(c["t"], c["K"], c["seed"], refine, among=among)) == raw(got), (name, with_among, refine)


def test_select_past_256_workgroup_counts(gpu_ctx):
    """65 537 voxels: compact()'s scan takes a second pass for the 257th count, and the emit kernel runs past 65 536
    points.  Everything; every other voxel; the 257th workgroup's one voxel alone; all but one, seeded."""
    m = pkg()
    c, cloud = cloud_of(m, gpu_ctx, "slab 65537")
    M = cloud.n_voxels
    assert M == 65537
    whole = columns(cloud.batch())
    assert np.array_equal(whole.view(np.uint32), c["vox"]["f32"].view(np.uint32))
    most = np.ones(M, bool)
    most[np.random.default_rng(65537).integers(M)] = False
    for mask in (np.ones(M, bool), np.arange(M) % 2 == 1, np.arange(M) >= 256 * 256, most):
        got = cloud.select(mask)
        assert got.n_points == int(mask.sum()) and got.n_frames == 1
        assert columns(got).tobytes() == whole[mask].tobytes(), int(mask.sum())
        assert columns(cloud.select(mask)).tobytes() == columns(got).tobytes()


def grid_cloud(m, ctx, c, src=None):
    """The build of a grid case on its own h and origin (src: a Batch of the same values) and its precondition: the
    keys and the bits of the rows are the restatement's."""
    cloud = m.voxel_downsample(c["rows"] if src is None else src, c["h"], c["origin"], context=ctx)
    assert np.array_equal(cloud.keys(), c["vox"]["keys"])
    assert np.array_equal(cloud.rows().view(np.uint64), c["vox"]["rows"].view(np.uint64))
    return cloud


def batch_of(ctx, rows):
    """The rows as a Batch of three frames, the middle one empty."""
    b = ctx.batch([100, 0, len(rows) - 100])
    b.upload_columns(*[rows[:, k].astype(np.float32) for k in range(4)])
    return b


@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_grids_off_the_default_origin(gpu_ctx, grid):
    """P.slab(257) on every grid of V.ORIGIN_GRIDS (a UTM-scale origin with the cloud there; an origin that is no
    multiple of h; far keys whose o + k h cancels; the same on h = 7.3): the build, the plane both ways and the
    selection of its inliers against the restatement, twice; and where float32 can hold the case, the Batch build
    and the rows build of the same float32 values give the same bytes."""
    m = pkg()
    ctx = gpu_ctx
    c = P.grid_case(grid)
    cloud = grid_cloud(m, ctx, c)
    whole = columns(cloud.batch())
    assert np.array_equal(whole.view(np.uint32), c["vox"]["f32"].view(np.uint32))
    for refine in (False, True):
        want = P.grid_expect(grid, refine)
        got = cloud.segment_plane(c["t"], c["K"], c["seed"], refine)
        print(f"{grid}: refine {refine}: iteration {got.iteration} ({want['iteration']}), score {got.score} ({want['score']}), "
              f"inliers {got.n_inliers} ({want['n_inliers']}), model {got.model.tolist()} ({want['model'].tolist()})")
        assert shapes_hold(got, cloud.n_voxels)
        assert P.equal(got, want, refine), (grid, refine)
        assert raw(cloud.segment_plane(c["t"], c["K"], c["seed"], refine)) == raw(got), (grid, refine)
        assert want["score"] >= 0.6 * cloud.n_voxels                      # the slab's plane, not a chance hit
        sel = columns(cloud.select(got.inliers))
        assert sel.tobytes() == whole[want["inliers"]].tobytes() == columns(cloud.select(got.inliers)).tobytes()
    if not V.ORIGIN_GRIDS[grid]["batch"]:
        return
    c = P.grid_case(grid, float32=True)
    seen = []
    for src in (None, batch_of(ctx, c["rows"])):
        cloud = grid_cloud(m, ctx, c, src)
        for refine in (False, True):
            got = cloud.segment_plane(c["t"], c["K"], c["seed"], refine)
            assert P.equal(got, P.grid_expect(grid, refine, float32=True), refine), (grid, refine, src is None)
            seen.append(raw(got))
        seen.append(columns(cloud.select(got.inliers)).tobytes())
    assert seen[:3] == seen[3:]


def test_peel_ground_then_wall_then_clusters(gpu_ctx):
    """Segment, segment again among what is left, cluster the rest: every step against its restatement."""
    m = pkg()
    c, cloud = cloud_of(m, gpu_ctx, "ground + wall")
    ground = cloud.segment_plane(c["t"], c["K"], c["seed"])
    assert P.equal(ground, P.expect("ground + wall", True), True) and ground.n_inliers == 300
    rest = ~ground.inliers
    for refine in (True, False):
        want = P.expect("ground + wall", refine, among=rest, key="rest")
        wall = cloud.segment_plane(c["t"], c["K"], c["seed"], refine, among=rest)
        assert P.equal(wall, want, refine), refine
        assert raw(cloud.segment_plane(c["t"], c["K"], c["seed"], refine, among=rest)) == raw(wall)
    assert wall.n_inliers == 150 and not (wall.inliers & ground.inliers).any() and abs(wall.model[0]) > 0.999
    left = rest & ~wall.inliers
    assert left.sum() == cloud.n_voxels - 450
    # among of fewer than three candidates
    few = np.zeros(cloud.n_voxels, bool)
    few[:2] = True
    with pytest.raises(ValueError, match="three candidate"):
        cloud.segment_plane(c["t"], among=few)
    # the wall as a cloud of its own: the selection, voxelised again on the same grid, clustered
    sel = cloud.select(wall.inliers)
    rows = columns(sel).astype(np.float64)
    assert np.array_equal(rows.astype(np.float32), c["vox"]["f32"][wall.inliers])
    again = m.voxel_downsample(sel, c["h"], context=gpu_ctx)
    d = V.downsample(rows, c["h"])
    want = C.dbscan(d["keys"], d["rows"][:, :3], d["counts"], c["h"], 2 * c["h"], 3, False)
    assert C.equal(again.clusters(2 * c["h"], 3), want) and want["K"] >= 1


def test_lifetime_and_timing(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    c, cloud = cloud_of(m, ctx, "ground + wall")
    M = cloud.n_voxels
    ground = cloud.segment_plane(c["t"], c["K"], c["seed"])
    ctx.read_timing_plane()
    ctx.timing(True)
    try:
        wall = cloud.segment_plane(c["t"], c["K"], c["seed"], among=~ground.inliers)
        cloud.select(wall.inliers)
    finally:
        ctx.timing(False)
    t = ctx.read_timing_plane()
    assert set(t) == {"compact_ms", "sample_ms", "score_ms", "mask_ms", "moments_ms", "select_ms", "regions"}
    assert all(t[k] > 0 for k in t), t
    assert t["regions"] == 8            # compact, sample, score, mask twice, moments, the selection's scan and emit
    assert ctx.read_timing_plane() == {"compact_ms": 0.0, "sample_ms": 0.0, "score_ms": 0.0, "mask_ms": 0.0,
                                       "moments_ms": 0.0, "select_ms": 0.0, "regions": 0}
    # normals and clusters share the build and its centroids with the plane, in either order
    name = "257 voxels"
    n = N.case(name)
    shared = m.voxel_downsample(n["rows"], n["h"], context=ctx)
    plane = shared.segment_plane(n["h"], 50, 1)
    cent = n["vox"]["rows"][:, :3]
    assert P.equal(plane, dict(P.ransac(cent, n["h"], 50, 1, True), cent=np.ascontiguousarray(cent)), True)
    assert np.array_equal(shared.normals(n["radius"]).counts, n["est"]["counts"])
    assert C.equal(shared.clusters(C.case(name)["eps"], 4), C.expect(name, 4))
    assert raw(shared.segment_plane(n["h"], 50, 1)) == raw(plane)
    # the C entries' own refusals
    lib, h = ctx.lib, ctx.handle
    cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
    model, samples, stats = np.zeros(4), np.zeros(3, np.int32), np.zeros(4, np.int64)
    out = (m._lib.ptr(model, ctypes.c_double), None, m._lib.ptr(samples, ctypes.c_int32), m._lib.ptr(stats, ctypes.c_int64))
    for dist, K, refine in ((0.0, 10, 1), (-1.0, 10, 1), (float("nan"), 10, 1), (float("inf"), 10, 1), (c["t"], 0, 1),
                            (c["t"], -5, 1), (c["t"], 2 ** 20 + 1, 1), (c["t"], 10, 2), (c["t"], 10, -1)):
        assert lib.mc_voxel_plane(h, dist, K, 0, refine, None, None, *out) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_plane(h, c["t"], 10, 0, 1, None, None, None, None, out[2], out[3]) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_plane(h, c["t"], 10, 0, 1, None, None, out[0], None, None, out[3]) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_plane(h, c["t"], 10, 0, 1, None, None, out[0], None, out[2], None) == m._lib.MC_ERR_INVALID
    few = ctx.device_buffer(M)
    few.from_host((np.arange(M) < 2).astype(np.uint8))
    assert lib.mc_voxel_plane(h, c["t"], 10, 0, 1, few.ptr, None, *out) == m._lib.MC_ERR_INVALID
    assert "three candidate" in lib.mc_last_error().decode()
    assert lib.mc_voxel_plane(h, c["t"], c["K"], c["seed"], 1, None, None, *out) == m._lib.MC_OK      # d_inliers and cov NULL
    assert stats.tolist() == [ground.iteration, ground.score, ground.n_inliers, 1]
    assert np.array_equal(model.view(np.uint64), ground.model.view(np.uint64)) and np.array_equal(samples, ground.samples)
    # fewer than three voxels, M = 0 among them
    two = m.voxel_downsample(P.case("slab 3")["rows"][:2], 0.25, context=ctx)
    assert lib.mc_voxel_plane(h, 0.25, 10, 0, 1, None, None, *out) == m._lib.MC_ERR_INVALID
    with pytest.raises(ValueError, match="three candidate"):
        two.segment_plane(0.25)
    none = m.voxel_downsample(np.zeros((0, 4)), 0.25, context=ctx)
    assert lib.mc_voxel_plane(h, 0.25, 10, 0, 1, None, None, *out) == m._lib.MC_ERR_INVALID
    with pytest.raises(ValueError, match="three candidate"):
        none.segment_plane(0.25)
    # a later build on the context ends the cloud; so does close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.segment_plane(c["t"])
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.select(np.ones(M, bool))
    none.close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        none.select(np.zeros(0, bool))
    assert lib.mc_voxel_plane(h, 0.25, 10, 0, 1, None, None, *out) == m._lib.MC_ERR_STATE
    assert lib.mc_voxel_emit_selected(h, few.ptr, ctx.batch([2]).handle) == m._lib.MC_ERR_STATE
