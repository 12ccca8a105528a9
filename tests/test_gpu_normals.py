"""The surface normals of a voxel cloud on the device (VoxelCloud.normals; csrc/normals.hpp) against the NumPy
restatement of tests/normals.py: neighbour counts and covariances bit for bit, normals and curvature by the
eigenvector criterion (C_BOUND there), the sign rule, and every case against a second run byte for byte."""
import ctypes

import numpy as np
import pytest

import normals as N
import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    return (np.array_equal(bits(a.normals), bits(b.normals)) and np.array_equal(bits(a.curvature), bits(b.curvature))
            and np.array_equal(a.counts, b.counts) and np.array_equal(bits(a.covariance), bits(b.covariance)))


def run_case(ctx, name, viewpoint=None):
    """The case through float64 rows: the cloud is the restatement's, the normals hold against it, twice."""
    m = pkg()
    c = N.case(name)
    cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
    assert np.array_equal(cloud.keys(), c["vox"]["keys"]) and np.array_equal(bits(cloud.rows()), bits(c["vox"]["rows"]))
    got = cloud.normals(c["radius"], c["max_nn"], viewpoint, covariance=True)
    M = cloud.n_voxels
    assert got.normals.shape == (M, 3) and got.curvature.shape == (M,) and got.covariance.shape == (M, 6)
    assert got.counts.dtype == np.int32 and got.normals.dtype == np.float64
    k = N.check_against(c["est"], got.normals, got.curvature, got.counts, got.covariance, viewpoint,
                        c["vox"]["rows"][:, :3], name)
    assert same(got, cloud.normals(c["radius"], c["max_nn"], viewpoint, covariance=True)), name
    if len(k["unit"]):
        print(f"{name}: unit {k['unit'].max():.2f}  rayleigh {k['rayleigh'].max():.3f}  curvature {k['curv'].max():.3f} "
              f"(bounds 8, {N.C_BOUND}, {N.C_BOUND})")
    return cloud, got, k


def test_plane_at_gps_scale(gpu_ctx):
    """The reference's own parameters (h = 0.05, radius = 0.1, max_nn = 30) at coordinates around 1000 m; the
    analytic normal within what the criterion and each voxel's eigenvalue gap imply."""
    c = N.case("plane")
    _, got, k = run_case(gpu_ctx, "plane")
    n = got.normals[k["sel"]]
    sine = np.linalg.norm(np.cross(n, N.PLANE_NORMAL), axis=1)
    bound = N.plane_angle_bound(k, c["h"])
    print(f"plane: largest sine / bound {float((sine / bound).max()):.3f}, median bound {np.median(bound):.2e}")
    assert (sine <= bound).all() and np.median(bound) < 1e-6
    assert (n @ N.PLANE_NORMAL > 0).all() and (got.curvature[k["sel"]] <= 1e-9).mean() > 0.9


def test_dense_block_takes_the_cap_with_ties_broken_by_key(gpu_ctx):
    inside = ((N.case("block")["vox"]["keys"] >= 2) & (N.case("block")["vox"]["keys"] <= 5)).all(axis=1)
    _, capped, _ = run_case(gpu_ctx, "block")
    assert (capped.counts[inside] == 30).all() and capped.counts.max() == 30
    _, free, _ = run_case(gpu_ctx, "block uncapped")
    assert (free.counts[inside] == 33).all()
    # the three neighbours dropped are +x, +y, +z at two cells: the covariance stays diagonal but its mean moves
    assert not np.array_equal(bits(capped.covariance[inside]), bits(free.covariance[inside]))


def test_isolated_voxels_and_a_collinear_triple(gpu_ctx):
    _, got, _ = run_case(gpu_ctx, "isolated")
    assert got.counts.tolist() == N.ISOLATED_COUNTS
    assert (got.normals[:3] == [0.0, 0.0, 1.0]).all() and (got.curvature[:3] == 0.0).all()
    # rank 1 along x: any perpendicular is right, and the curvature is exactly 0
    assert (got.normals[3:, 0] == 0.0).all() and (got.curvature[3:] == 0.0).all()
    # below three neighbours a viewpoint changes nothing
    _, down, _ = run_case(gpu_ctx, "isolated", (0.0, 0.0, -50.0))
    assert (down.normals[:3] == [0.0, 0.0, 1.0]).all()


def test_key_range_ends_do_not_wrap(gpu_ctx):
    _, got, _ = run_case(gpu_ctx, "key ends")
    assert got.counts.tolist() == N.key_ends()[3]


@pytest.mark.parametrize("name", ["30 voxels", "257 voxels", "70001 voxels"])
def test_chains_and_sizes(gpu_ctx, name):
    """30 voxels: the 64-slot table, where probes walk chains; 257: a ragged last workgroup; 70 001: more than
    one wave per SIMD."""
    run_case(gpu_ctx, name)


def by_key(cloud, got):
    order = np.argsort(V.pack(cloud.keys()))
    return [np.ascontiguousarray(a[order]) for a in (cloud.keys(), got.normals, got.curvature, got.counts, got.covariance)]


def test_order_independence_and_both_sources(gpu_ctx):
    """The same points in another order and split differently into frames, as a Batch and as float64 rows: per
    packed key the same normal, curvature, count and covariance, bit for bit."""
    m = pkg()
    ctx = gpu_ctx
    rng = np.random.default_rng(66)
    centre = rng.integers(-20, 20, (1500, 3)) * [1, 1, 0]
    pick = np.concatenate([np.arange(1500), rng.integers(0, 1500, 4500)])
    rows = np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (6000, 3))) * 0.2, rng.uniform(0, 1, 6000)])
    rows = rows.astype(np.float32).astype(np.float64)          # values a batch can hold
    d, est = N.of_rows(rows, 0.2, 0.4)
    assert 900 < len(d["rows"]) <= 1500 and est["counts"].max() >= 10 and est["counts"].min() < 3
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
        got = cloud.normals(0.4, covariance=True)
        if not shuffle and source == "rows":
            N.check_against(est, got.normals, got.curvature, got.counts, got.covariance, what="order, as given")
        seen.append(by_key(cloud, got))
    for other in seen[1:]:
        assert np.array_equal(other[0], seen[0][0]) and np.array_equal(other[3], seen[0][3])
        for a, b in zip(other, seen[0]):
            assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["R = 1", "R = 4", "R = 4 at the fewest", "R = 4 at the most"])
def test_window_ends(gpu_ctx, name):
    """radius = 0.9 h: the 27-cell window; radius = 4 h: 729 cells, where the cap applies to most voxels, at
    max_nn = 30 and at both ends of its range."""
    c = N.case(name)
    assert c["est"]["R"] == (1 if name == "R = 1" else 4)
    run_case(gpu_ctx, name)


def grid_run(ctx, c, src=None):
    """run_case for a grid case: built on its own h and origin (src: a Batch of the same values)."""
    m = pkg()
    cloud = m.voxel_downsample(c["rows"] if src is None else src, c["h"], c["origin"], context=ctx)
    assert np.array_equal(cloud.keys(), c["vox"]["keys"]) and np.array_equal(bits(cloud.rows()), bits(c["vox"]["rows"]))
    got = cloud.normals(c["radius"], c["max_nn"], covariance=True)
    k = N.check_against(c["est"], got.normals, got.curvature, got.counts, got.covariance, None, c["vox"]["rows"][:, :3])
    assert same(got, cloud.normals(c["radius"], c["max_nn"], covariance=True))
    return got, k


@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_grids_off_the_default_origin(gpu_ctx, grid):
    """The 257-point slab on every grid of V.ORIGIN_GRIDS (a UTM-scale origin with the cloud there; an origin that is
    no multiple of h; far keys whose o + k h cancels; the same on h = 7.3), at radius 2 h and 4 h: the build is the
    restatement's, counts and covariance equal bit for bit, the normals hold the criterion, twice.  Where float32
    can hold the case, the Batch build and the rows build of the same float32 values give the same bytes."""
    for rel in (2.0, 4.0):
        c = N.grid_case(grid, rel)
        got, k = grid_run(gpu_ctx, c)
        assert (got.counts >= 3).sum() >= 200              # the slab is a quarter occupied: nearly every voxel has neighbours
        print(f"{grid}: radius {rel} h: {len(got.counts)} voxels, unit {k['unit'].max():.2f}  rayleigh {k['rayleigh'].max():.3f}  "
              f"curvature {k['curv'].max():.3f} (bounds 8, {N.C_BOUND}, {N.C_BOUND})")
    if V.ORIGIN_GRIDS[grid]["batch"]:
        c = N.grid_case(grid, float32=True)
        b = gpu_ctx.batch([100, 0, len(c["rows"]) - 100])
        b.upload_columns(*[c["rows"][:, k].astype(np.float32) for k in range(4)])
        from_rows, _ = grid_run(gpu_ctx, c)
        from_batch, _ = grid_run(gpu_ctx, c, b)
        assert same(from_rows, from_batch)


def test_a_radius_beyond_four_voxels_is_refused(gpu_ctx):
    m = pkg()
    c = N.case("257 voxels")
    cloud = m.voxel_downsample(c["rows"], c["h"], context=gpu_ctx)
    with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
        cloud.normals(4.01 * c["h"])
    buf = gpu_ctx.device_buffer(32 * cloud.n_voxels)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    assert lib.mc_voxel_normals(h, 4.01 * c["h"], 30, None, buf.ptr, None, None) == m._lib.MC_ERR_INVALID
    assert "voxelise coarser or shrink the radius" in lib.mc_last_error().decode()
    vp = np.array([0.0, np.nan, 0.0])
    for radius, max_nn, view in ((0.0, 30, None), (-1.0, 30, None), (float("nan"), 30, None), (float("inf"), 30, None),
                                 (0.4, 2, None), (0.4, 65, None), (0.4, -1, None), (0.4, 30, vp)):
        assert lib.mc_voxel_normals(h, radius, max_nn, m._lib.ptr(view, ctypes.c_double), buf.ptr, None,
                                    None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_normals(h, 4.0 * c["h"], 0, None, buf.ptr, None, None) == m._lib.MC_OK


def test_viewpoint_on_either_side_flips_every_normal(gpu_ctx):
    _, above, k = run_case(gpu_ctx, "plane", (1000.9, 1000.9, 1000.0))
    _, below, _ = run_case(gpu_ctx, "plane", (1000.9, 1000.9, -1000.0))
    sel = k["sel"]
    assert sel.sum() > 1300
    assert np.array_equal(bits(above.normals[sel]), bits(-below.normals[sel]))
    assert (above.normals[sel] @ N.PLANE_NORMAL > 0).all() and (below.normals[sel] @ N.PLANE_NORMAL < 0).all()
    assert np.array_equal(bits(above.curvature), bits(below.curvature)) and np.array_equal(above.counts, below.counts)
    assert np.array_equal(bits(above.normals[~sel]), bits(below.normals[~sel]))       # (0, 0, 1) either way


def test_lifetime_and_timing(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    c = N.case("block")
    ctx.read_timing_normals()
    ctx.timing(True)
    try:
        cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
        wide = cloud.normals(1.0)                              # centroids, window, cap
        narrow = cloud.normals(0.5, covariance=True)           # window (seven neighbours at the most: no cap launch)
        free = cloud.normals(1.0, max_nn=0)                    # window
    finally:
        ctx.timing(False)
    t = ctx.read_timing_normals()
    assert t["regions"] == 5 and t["centroids_ms"] > 0 and t["window_ms"] > 0 and t["cap_ms"] > 0
    assert set(t) == {"centroids_ms", "window_ms", "cap_ms", "regions"}
    assert ctx.read_timing_normals() == {"centroids_ms": 0.0, "window_ms": 0.0, "cap_ms": 0.0, "regions": 0}
    assert wide.covariance is None and narrow.covariance.shape == (512, 6)
    assert np.array_equal(wide.counts, c["est"]["counts"]) and narrow.counts.max() == 7 and free.counts.max() == 33
    est = N.estimate(c["vox"]["keys"], c["vox"]["rows"][:, :3], c["h"], 0.5)
    N.check_against(est, narrow.normals, narrow.curvature, narrow.counts, narrow.covariance, what="second radius")
    # a later build on the context ends the cloud; so does close()
    later = m.voxel_downsample(N.case("isolated")["rows"], 0.5, context=ctx)
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.normals(1.0)
    assert later.normals(1.0).counts.tolist() == N.ISOLATED_COUNTS
    later.close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        later.normals(1.0)
    buf = ctx.device_buffer(64)
    assert ctx.lib.mc_voxel_normals(ctx.handle, 1.0, 30, None, buf.ptr, None, None) == m._lib.MC_ERR_STATE
    empty = m.voxel_downsample(np.zeros((0, 4)), 0.1, context=ctx).normals(0.2, covariance=True)
    assert empty.normals.shape == (0, 3) and empty.curvature.shape == (0,) and empty.counts.shape == (0,)
    assert empty.covariance.shape == (0, 6) and empty.counts.dtype == np.int32
