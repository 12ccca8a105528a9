"""The density clustering of a voxel cloud on the device (VoxelCloud.clusters; csrc/cluster.hpp) against the
NumPy / scipy restatement of tests/clusters.py.  Every output is an integer, so every comparison is exact: labels,
densities, K and the four stats arrays equal the restatement's, and a second call equals the first byte for byte —
although the components are built with atomics."""
import ctypes

import numpy as np
import pytest

import clusters as C
import normals as N
import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def raw(r):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (r.labels, r.density, r.voxels, r.points, r.cell_min, r.cell_max))


def shapes_hold(r, M):
    K = r.n_clusters
    return (r.labels.shape == (M,) and r.density.shape == (M,) and r.voxels.shape == (K,) and r.points.shape == (K,)
            and r.cell_min.shape == (K, 3) and r.cell_max.shape == (K, 3) and isinstance(K, int)
            and [a.dtype for a in r[:2] + r[3:]] == [np.int32, np.int32, np.int32, np.int64, np.int32, np.int32])


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_cloud_equals_the_restatement_twice(gpu_ctx, name):
    """tie: a border voxel between two cores at exactly eps joins the lower key, whichever block came first;
    isolated: d2 == eps2 is inside, one ulp less is not; chain: the deep tree of find; contention: six unions per
    voxel into one component; the slabs: the 64-slot table's chains, a ragged last workgroup, many workgroups,
    R = 1 and R = 4; key ends: a window cell outside the key range links nothing; weighted: the density is the
    neighbours' source points."""
    m = pkg()
    c = C.case(name)
    cloud = m.voxel_downsample(c["rows"], c["h"], context=gpu_ctx)
    assert np.array_equal(cloud.keys(), c["vox"]["keys"]) and np.array_equal(cloud.point_counts(), c["vox"]["counts"])
    for min_points, weighted in c["runs"]:
        want = C.expect(name, min_points, weighted)
        got = cloud.clusters(c["eps"], min_points, weighted)
        print(f"{name}: min_points {min_points} weighted {weighted}: K {got.n_clusters} (restatement {want['K']}), noise "
              f"{int((got.labels < 0).sum())}, labels differing {int((got.labels != want['labels']).sum())}, densities "
              f"differing {int((got.density != want['density']).sum())}")
        assert shapes_hold(got, cloud.n_voxels)
        assert C.equal(got, want), (name, min_points, weighted)
        assert raw(cloud.clusters(c["eps"], min_points, weighted)) == raw(got), (name, min_points, weighted)


@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_grids_off_the_default_origin(gpu_ctx, grid):
    """The 257-point slab on every grid of V.ORIGIN_GRIDS (a UTM-scale origin with the cloud there; an origin that is
    no multiple of h; far keys whose o + k h cancels; the same on h = 7.3) at eps = 2 h: the build is the
    restatement's and every run of C.GRID_RUNS equals it, twice.  Where float32 can hold the case, the Batch build
    and the rows build of the same float32 values give the same bytes."""
    m = pkg()
    ctx = gpu_ctx
    for float32 in ((False, True) if V.ORIGIN_GRIDS[grid]["batch"] else (False,)):
        c = C.grid_case(grid, float32)
        sources = [c["rows"]]
        if float32:
            b = ctx.batch([100, 0, len(c["rows"]) - 100])
            b.upload_columns(*[c["rows"][:, k].astype(np.float32) for k in range(4)])
            sources.append(b)
        seen = []
        for src in sources:
            cloud = m.voxel_downsample(src, c["h"], c["origin"], context=ctx)
            assert np.array_equal(cloud.keys(), c["vox"]["keys"]) and np.array_equal(cloud.point_counts(), c["vox"]["counts"])
            assert np.array_equal(cloud.rows().view(np.uint64), c["vox"]["rows"].view(np.uint64))
            for min_points, weighted in c["runs"]:
                want = C.grid_expect(grid, min_points, weighted, float32)
                got = cloud.clusters(c["eps"], min_points, weighted)
                print(f"{grid}: float32 {float32} min_points {min_points} weighted {weighted}: K {got.n_clusters} "
                      f"(restatement {want['K']}), labels differing {int((got.labels != want['labels']).sum())}")
                assert shapes_hold(got, cloud.n_voxels)
                assert C.equal(got, want), (grid, min_points, weighted)
                assert raw(cloud.clusters(c["eps"], min_points, weighted)) == raw(got), (grid, min_points, weighted)
                seen.append(raw(got))
        assert len(sources) == 1 or seen[:3] == seen[3:]
        assert C.grid_expect(grid, 4, False, float32)["K"] >= 2              # clusters, noise and borders to tell apart


def by_key(cloud, got):
    """Per packed key, ascending: the key, the density, and the lowest packed key of the voxel's cluster (-1: noise)."""
    packed = V.pack(cloud.keys())
    low = np.full(max(got.n_clusters, 1), np.iinfo(np.int64).max, np.int64)
    on = got.labels >= 0
    np.minimum.at(low, got.labels[on], packed[on])
    lowest = np.where(on, low[np.maximum(got.labels, 0)], -1)
    order = np.argsort(packed)
    return packed[order], got.density[order], lowest[order]


@pytest.mark.parametrize("min_points,weighted", [(1, False), (8, False), (40, True)])
def test_order_independence_and_both_sources(gpu_ctx, min_points, weighted):
    """The same points in another order and split differently into frames, as a Batch and as float64 rows: per
    packed key the same density and the same cluster (named by its lowest key), and in every run the labels are
    the canonical numbering of that run's order."""
    m = pkg()
    ctx = gpu_ctx
    rng = np.random.default_rng(66)
    centre = rng.integers(-20, 20, (1500, 3)) * [1, 1, 0]
    pick = np.concatenate([np.arange(1500), rng.integers(0, 1500, 4500)])
    rows = np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (6000, 3))) * 0.2, rng.uniform(0, 1, 6000)])
    rows = rows.astype(np.float32).astype(np.float64)          # values a batch can hold
    d = V.downsample(rows, 0.2)
    want = C.dbscan(d["keys"], d["rows"][:, :3], d["counts"], 0.2, 0.4, min_points, weighted)
    assert 900 < len(d["keys"]) <= 1500
    if min_points > 1:      # 17 and 9 clusters, with noise and border voxels; at min_points = 1 one component
        assert want["K"] >= 9 and (want["labels"] < 0).sum() > 50 and ((want["labels"] >= 0) & ~want["core"]).sum() > 50
    seen = []
    for source, counts, shuffle in (("rows", None, False), ("rows", None, True), ("batch", [6000], False),
                                    ("batch", [1000, 0, 2499, 2501], True), ("batch", [1] * 7 + [5993], True)):
        r = rows[rng.permutation(len(rows))] if shuffle else rows
        if source == "batch":
            b = ctx.batch(counts)
            b.upload_columns(*[r[:, c].astype(np.float32) for c in range(4)])
            cloud = ctx.voxel_downsample(b, 0.2)
        else:
            cloud = m.voxel_downsample(r, 0.2, context=ctx)
        got = cloud.clusters(0.4, min_points, weighted)
        if not shuffle and source == "rows":
            assert C.equal(got, want)
        assert got.n_clusters == want["K"] and C.canonical(got.labels, got.density >= min_points)
        assert got.voxels.sum() == (got.labels >= 0).sum() and np.array_equal(np.bincount(got.labels[got.labels >= 0]), got.voxels)
        seen.append(by_key(cloud, got))
    for other in seen[1:]:
        for a, b in zip(other, seen[0]):
            assert np.array_equal(a, b)


def test_lifetime_and_timing(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    name = "257 voxels"
    c = C.case(name)
    ctx.read_timing_clusters()
    ctx.timing(True)
    try:
        cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
        four = cloud.clusters(c["eps"], 4)
        ten = cloud.clusters(c["eps"], 10)
    finally:
        ctx.timing(False)
    t = ctx.read_timing_clusters()
    assert set(t) == {"density_ms", "union_ms", "label_ms", "number_ms", "stats_ms", "regions"}
    assert t["regions"] == 10 and all(t[k] > 0 for k in t)
    assert ctx.read_timing_clusters() == {"density_ms": 0.0, "union_ms": 0.0, "label_ms": 0.0, "number_ms": 0.0,
                                          "stats_ms": 0.0, "regions": 0}
    assert C.equal(four, C.expect(name, 4)) and C.equal(ten, C.expect(name, 10))
    # the stats follow the last call
    K = ten.n_clusters
    assert K == 6 != four.n_clusters
    lib, h = ctx.lib, ctx.handle
    buf = ctx.device_buffer(4 * K)
    assert lib.mc_voxel_cluster_stats(h, buf.ptr, None, None, None) == m._lib.MC_OK
    assert np.array_equal(buf.to_host(np.int32, count=K), ten.voxels)
    # the normals and the clustering share the build and its centroids, in either order
    assert np.array_equal(cloud.normals(c["eps"]).counts, N.case(name)["est"]["counts"])
    assert C.equal(cloud.clusters(c["eps"], 4), C.expect(name, 4))
    # the C entries' own refusals
    M = cloud.n_voxels
    lab = ctx.device_buffer(4 * M)
    for eps, min_points, weighted in ((0.0, 4, 0), (-1.0, 4, 0), (float("nan"), 4, 0), (float("inf"), 4, 0),
                                      (4.01 * c["h"], 4, 0), (c["eps"], 0, 0), (c["eps"], -3, 0), (c["eps"], 4, 2),
                                      (c["eps"], 4, -1)):
        assert lib.mc_voxel_clusters(h, eps, min_points, weighted, lab.ptr, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_clusters(h, 4.01 * c["h"], 4, 0, lab.ptr, None, None) == m._lib.MC_ERR_INVALID
    assert "voxelise coarser or shrink the radius" in lib.mc_last_error().decode()
    assert lib.mc_voxel_clusters(h, c["eps"], 4, 0, None, None, None) == m._lib.MC_ERR_INVALID      # d_labels NULL, M > 0
    with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
        cloud.clusters(4.01 * c["h"])
    k = ctypes.c_int64(-1)
    assert lib.mc_voxel_clusters(h, 4.0 * c["h"], 4, 0, lab.ptr, None, ctypes.byref(k)) == m._lib.MC_OK and k.value >= 1
    # a later build on the context ends the cloud and its clustering; so does close()
    later = m.voxel_downsample(N.isolated()[0], 0.5, context=ctx)
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.clusters(c["eps"], 4)
    assert lib.mc_voxel_cluster_stats(h, buf.ptr, None, None, None) == m._lib.MC_ERR_STATE       # no clustering of this build
    assert later.clusters(1.0, 3).labels.tolist() == [-1, -1, -1, 0, 0, 0]
    later.close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        later.clusters(1.0, 3)
    assert lib.mc_voxel_clusters(h, 1.0, 3, 0, lab.ptr, None, None) == m._lib.MC_ERR_STATE
    assert lib.mc_voxel_cluster_stats(h, buf.ptr, None, None, None) == m._lib.MC_ERR_STATE


def test_empty_one_voxel_and_all_noise(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    cloud = m.voxel_downsample(np.zeros((0, 4)), 0.1, context=ctx)
    empty = cloud.clusters(0.2)
    assert shapes_hold(empty, 0) and empty.n_clusters == 0
    k = ctypes.c_int64(-1)
    assert ctx.lib.mc_voxel_clusters(ctx.handle, 0.2, 10, 0, None, None, ctypes.byref(k)) == m._lib.MC_OK and k.value == 0
    assert ctx.lib.mc_voxel_cluster_stats(ctx.handle, None, None, None, None) == m._lib.MC_OK
    one = m.voxel_downsample(np.array([[1.23, -4.5, 0.7, 0.5]] * 3), 0.1, context=ctx)
    alone = one.clusters(0.2, 1)
    assert shapes_hold(alone, 1) and alone.labels.tolist() == [0] and alone.density.tolist() == [1] and alone.n_clusters == 1
    assert alone.voxels.tolist() == [1] and alone.points.tolist() == [3]
    assert np.array_equal(alone.cell_min, one.keys()) and np.array_equal(alone.cell_max, one.keys())
    heavy = one.clusters(0.2, 3, weighted=True)
    assert heavy.labels.tolist() == [0] and heavy.density.tolist() == [3]
    noise = one.clusters(0.2, 2)
    assert shapes_hold(noise, 1) and noise.labels.tolist() == [-1] and noise.n_clusters == 0 and noise.voxels.shape == (0,)
    c = C.case("257 voxels")
    far = m.voxel_downsample(c["rows"], c["h"], context=ctx).clusters(c["eps"], 100)
    assert shapes_hold(far, 257) and far.n_clusters == 0 and (far.labels == -1).all() and far.points.shape == (0,)
    assert np.array_equal(far.density, C.expect("257 voxels", 10)["density"])
