"""The plane segmentation of a voxel cloud without a GPU: (1) csrc/plane_core.hpp compiles alone behind the
stand-ins; (2) the scalar core, included by tests/host/plane_host.cpp, built with g++ plainly and under
ASan + UBSan, against the NumPy restatement of tests/planes.py on every cloud — score table, winner, samples, masks,
the nine tree sums and the covariance bit for bit, the refit's normal by the eigenvector criterion, d^ recomputed from
the returned normal; (3) the sampler; (4) what the builder clouds promise, and a least-squares fit that does not
share the definition; (5) the module surface that needs no device.  Under (2) also the multi-level tree at 32 769 and
65 537 voxels and the grids off the default origin (tests/voxel.py ORIGIN_GRIDS)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hostbuild
import normals as N
import planes as P
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


# ---- (1) the core header on its own --------------------------------------------------------------------------------
@needs_gxx
def test_core_header_is_self_contained(tmp_path):
    """tests/test_core_headers.py's line on plane_core.hpp itself."""
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "device_standins.hpp"\n#include "plane_core.hpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", hostbuild.CSRC, "-I", hostbuild.HOST,
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(os.path.join(hostbuild.CSRC, "plane_core.hpp")).read()
    assert not [i for i in re.findall(r"#include\s+[<\"]([^>\"]+)", text) if "hip" in i.lower()]


# ---- (2) the core under g++ ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plane_host")
    return tmp, [hostbuild.build(tmp, "plane_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


def run_host(exe, tmp, cent, t, K, seed, refine, among=None):
    src, dst = tmp / "in.bin", tmp / "out.bin"
    M = len(cent)
    head = np.array([K, seed, int(refine), M, int(among is not None)], np.uint64).tobytes()
    src.write_bytes(np.float64(t).tobytes() + head + np.ascontiguousarray(cent, np.float64).tobytes()
                    + (b"" if among is None else np.ascontiguousarray(among, np.uint8).tobytes()))
    hostbuild.run(exe, src, dst)
    raw = dst.read_bytes()
    at = 8 * K
    stats = np.frombuffer(raw, "<i8", 4, at)
    out = dict(scores=np.frombuffer(raw, "<i8", K, 0), iteration=int(stats[0]), score=int(stats[1]), n_inliers=int(stats[2]),
               refined=bool(stats[3]), samples=np.frombuffer(raw, "<i4", 3, at + 32), model=np.frombuffer(raw, "<f8", 4, at + 48),
               covariance=np.frombuffer(raw, "<f8", 6, at + 80), sums=np.frombuffer(raw, "<f8", 9, at + 128),
               hyp_inliers=np.frombuffer(raw, np.uint8, M, at + 200).astype(bool),
               inliers=np.frombuffer(raw, np.uint8, M, at + 200 + M).astype(bool))
    assert len(raw) == at + 200 + 2 * M
    return out, raw


def runs():
    for name in P.CASES:
        for t in P.thresholds(name):
            for refine in (False, True):
                yield name, t, refine, None
    yield "slab 257", None, True, pkg().voxel.plane_score_chunk() + 1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@needs_gxx
def test_core_equals_the_restatement_on_every_cloud(exes):
    tmp, builds = exes
    for name, t, refine, K in runs():
        c = P.case(name)
        t = c["t"] if t is None else t
        K = c["K"] if K is None else K
        want = P.expect(name, refine, t, K)
        seen = []
        for exe in builds:
            got, raw = run_host(exe, tmp, c["cent"], t, K, c["seed"], refine)
            seen.append(raw)
            what = (name, t, refine, K)
            assert np.array_equal(got["scores"], want["scores"]), what
            assert np.array_equal(got["hyp_inliers"], want["hyp_inliers"]), what
            assert P.equal(got, want, refine), what
            if want["refined"]:
                assert np.array_equal(bits(got["sums"]), bits(want["sums"])), what
        assert seen[0] == seen[1], (name, t, refine)


@needs_gxx
def test_core_with_candidates_peels_the_wall(exes):
    tmp, builds = exes
    c = P.case("ground + wall")
    ground = P.expect("ground + wall", True)
    rest = ~ground["inliers"]
    for refine in (False, True):
        want = P.expect("ground + wall", refine, among=rest, key="rest")
        for exe in builds:
            got, _ = run_host(exe, tmp, c["cent"], c["t"], c["K"], c["seed"], refine, rest)
            assert np.array_equal(got["scores"], want["scores"]) and P.equal(got, want, refine)
            if refine:
                assert np.array_equal(bits(got["sums"]), bits(want["sums"]))


def hold(builds, tmp, c, want, refine, among=None, what=None):
    """Both builds of the core on a case's centroids against the restatement `want`, as the tests above."""
    seen = []
    for exe in builds:
        got, raw = run_host(exe, tmp, c["cent"], c["t"], c["K"], c["seed"], refine, among)
        seen.append(raw)
        assert np.array_equal(got["scores"], want["scores"]), what
        assert np.array_equal(got["hyp_inliers"], want["hyp_inliers"]), what
        assert P.equal(got, want, refine), what
        if want["refined"]:
            assert np.array_equal(bits(got["sums"]), bits(want["sums"])), what
    assert seen[0] == seen[1], what


@needs_gxx
@pytest.mark.parametrize("name", ["slab 32769", "slab 65537"])
def test_core_holds_the_multi_level_tree(exes, name):
    """32 769 voxels: 65 536 leaves, half of them padding, the smallest tree the device sums in more than one level;
    65 537: 131 072 leaves.  plane_tree against tests/planes.py's tree without a GPU: the nine sums bit for bit, with
    and without candidates."""
    tmp, builds = exes
    c = P.case(name)
    M = len(c["cent"])
    assert M == int(name.split()[1]) and P.plane_leaves_of(M) == 2 * (M - 1)
    for refine in (False, True):
        hold(builds, tmp, c, P.expect(name, refine), refine, what=(name, refine))
    among = P.among_of(M)
    hold(builds, tmp, c, P.expect(name, True, among=among, key="among"), True, among, what=(name, "among"))


@needs_gxx
@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_core_on_grids_off_the_default_origin(exes, grid):
    """The core takes centroids: those of V.downsample(rows, h, origin) on every grid of V.ORIGIN_GRIDS."""
    tmp, builds = exes
    c = P.grid_case(grid)
    assert np.array_equal(c["cent"], V.downsample(c["rows"], c["h"], c["origin"])["rows"][:, :3]) and 237 <= len(c["cent"]) <= 257
    if V.ORIGIN_GRIDS[grid]["moved"]:
        assert np.abs(c["cent"] - c["origin"]).max() < 1000.0 < np.abs(c["cent"]).max()
    for refine in (False, True):
        hold(builds, tmp, c, P.grid_expect(grid, refine), refine, what=(grid, refine))


# ---- (3) the sampler -----------------------------------------------------------------------------------------------
@needs_gxx
def test_sampler_draws_three_distinct_places(exes):
    tmp, builds = exes
    for n in (3, 4, 2 ** 31 - 1):
        for exe in builds:
            hostbuild.run(exe, "sampler", n, 10_000)
        for seed in (0, 2 ** 64 - 1):
            at = P.sample(seed, 10_000, n)
            assert (at >= 0).all() and (at < n).all()
            assert (at[:, 0] != at[:, 1]).all() and (at[:, 0] != at[:, 2]).all() and (at[:, 1] != at[:, 2]).all()
    # every place is drawn, and the three draws of n = 3 are every permutation
    assert len(np.unique(P.sample(1, 10_000, 3), axis=0)) == 6
    assert np.array_equal(np.unique(P.sample(1, 10_000, 257)), np.arange(257))
    assert P.mix(np.array([0], np.uint64))[0] == 0 and int(P.mix(np.array([1], np.uint64))[0]) == 0x5692161D100B05E5


# ---- (4) what the builder clouds promise ---------------------------------------------------------------------------
def test_builder_clouds_hold_what_they_promise():
    for name in P.SLABS:
        c = P.case(name)
        M, t = len(c["cent"]), c["t"]
        assert M == int(name.split()[1]) and np.ptp(c["cent"], axis=0).max() <= 64.0
        dist = np.abs((c["cent"] @ P.SLAB_NORMAL) - P.SLAB_NORMAL[2])              # to z = 0.3 x - 0.2 y + 1
        on = dist <= 0.6 * t
        assert on.sum() >= 0.6 * M and (dist[~on] >= 2 * t).all(), name
        e = P.expect(name, True)
        assert e["refined"] and np.array_equal(e["inliers"], on) and np.array_equal(e["hyp_inliers"], on), name
        # no voxel near the refined plane's edge, and a normal determined far better than the margin needs: the
        # refit's normal may differ from eigh's by angle_bound, over the extent (64 m) below 1e-4 m
        assert P.margin(e, t) >= 0.3 * t, (name, P.margin(e, t) / t)
        bound, F, gap = P.angle_bound(e["covariance"])
        assert gap >= F / 64 and bound * 64.0 < 1e-4 < 0.3 * t, (name, bound, gap / F)
    assert P.plane_leaves_of(1281) == 2048
    # two equal planes: both planes hold the top score; the lowest k wins
    c, e = P.case("two equal planes"), P.expect("two equal planes", False)
    top = np.flatnonzero(e["scores"] == e["scores"].max())
    assert e["score"] == 40 and e["iteration"] == top[0] and len(top) >= 2
    ids = np.arange(80)
    z_of = [c["cent"][ids[P.sample(c["seed"], c["K"], 80)[k]], 2] for k in top]
    planes_hit = {float(z[0]) for z in z_of if z[0] == z[1] == z[2]}
    assert planes_hit == {0.125, 5.125} and len(z_of) == len([z for z in z_of if z[0] == z[1] == z[2]])
    assert e["model"][:3].tolist() == [0.0, 0.0, 1.0] and e["model"][3] in (-0.125, -5.125)
    # collinear: no valid hypothesis
    for refine in (False, True):
        e = P.expect("collinear", refine)
        assert not e["valid"].any() and e["iteration"] == -1 and not e["inliers"].any() and not e["model"].any()
        assert e["n_inliers"] == 0 and e["score"] == 0 and not e["refined"] and e["covariance"] is None
    # the dyadic edge: exact products, the voxel at exactly t inside, the next centroid above it outside; at the
    # float64 below t the voxel at t (the next float64 above the threshold) is outside
    c = P.case("dyadic edge")
    xy = c["cent"][:, :2] * 256.0
    assert np.array_equal(xy, np.rint(xy)) and np.abs(c["cent"][:, :2]).max() <= 2.0
    assert c["cent"][24, 2] == P.EDGE_T and c["cent"][25, 2] == P.EDGE_T + 2.0 ** -34 and (c["cent"][:24, 2] == 0.0).all()
    t, under = P.thresholds("dyadic edge")
    assert under < t and np.nextafter(under, 1.0) == t == c["cent"][24, 2]
    at, below = P.expect("dyadic edge", False, t), P.expect("dyadic edge", False, under)
    for e in (at, below):
        assert e["model"][:3].tolist() == [0.0, 0.0, 1.0] and e["model"][3] == 0.0 and e["inliers"][:24].all()
        assert not e["inliers"][25:].any()
    assert at["inliers"][24] and at["score"] == 25 and not below["inliers"][24] and below["score"] == 24
    # ground + wall: the ground first, the wall among the rest
    c = P.case("ground + wall")
    ground = P.expect("ground + wall", True)
    wall = P.expect("ground + wall", True, among=~ground["inliers"], key="rest")
    assert ground["n_inliers"] == 300 and abs(ground["model"][2]) > 0.999 and abs(ground["model"][3]) < c["t"]
    assert wall["n_inliers"] == 150 and abs(wall["model"][0]) > 0.999 and not (wall["inliers"] & ground["inliers"]).any()
    assert abs(wall["model"][3] + 6.0) < c["t"]
    for e, cand in ((ground, None), (wall, ~ground["inliers"])):
        assert P.margin(e, c["t"], cand) >= 0.3 * c["t"]


def test_least_squares_agrees_on_the_slabs():
    """A fit that shares nothing with the definition — no tree sums, no covariance about p0, no Jacobi: the
    orthogonal least-squares plane of the slab's known inliers from numpy's SVD of the coordinates about their
    mean.  Its normal agrees with the restatement's within the criterion's angle bound, and the plane passes
    through the same centre."""
    for name in P.SLABS:
        c, e = P.case(name), P.expect(name, True)
        dist = np.abs((c["cent"] @ P.SLAB_NORMAL) - P.SLAB_NORMAL[2])
        pts = c["cent"][dist <= 0.6 * c["t"]]
        mean = pts.mean(axis=0)
        n = np.linalg.svd(pts - mean)[2][-1]
        bound = P.angle_bound(e["covariance"])[0]
        assert np.linalg.norm(np.cross(n, e["model"][:3])) <= bound, (name, bound)
        assert abs(e["model"][:3] @ mean + e["model"][3]) <= 64.0 * bound


# ---- (5) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_plane", "mc_voxel_plane_chunk", "mc_voxel_emit_selected", "mc_timing_read_plane")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def test_argument_errors_need_no_device():
    m = pkg()
    cloud = m.VoxelCloud(_NoDevice(), 10, 7, 0.05)
    for t in (0, 0.0, -0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="distance_threshold"):
            cloud.segment_plane(t)
    for K in (0, -1, 10.0, "10", None, True, False, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="num_iterations"):
            cloud.segment_plane(0.1, K)
    for seed in (-1, 2 ** 64, 1.0, "0", None, True):
        with pytest.raises(ValueError, match="seed"):
            cloud.segment_plane(0.1, 10, seed)
    for refine in (0, 1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="refine"):
            cloud.segment_plane(0.1, 10, 0, refine)
    good = np.ones(10, bool)
    for mask in (np.ones(9, bool), np.ones((10, 1), bool), np.ones(10, np.uint8), np.ones(10), [True] * 10, None):
        if mask is not None:
            with pytest.raises(ValueError, match="among"):
                cloud.segment_plane(0.1, among=mask)
        with pytest.raises(ValueError, match="mask"):
            cloud.select(mask)
    closed = m.VoxelCloud(_NoDevice(), 10, 6, 0.05)      # not the context's live generation
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.segment_plane(0.1)
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.segment_plane(np.float32(0.1), np.int64(2 ** 20), np.uint64(2 ** 64 - 1), np.True_, good)
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.select(good)
    assert m.VoxelPlane is m.voxel.VoxelPlane
    assert m.VoxelPlane._fields == ("model", "inliers", "n_inliers", "score", "iteration", "samples", "covariance", "refined")
    assert callable(m.VoxelCloud.segment_plane) and callable(m.VoxelCloud.select) and callable(m.Context.read_timing_plane)
    assert "VoxelPlane" in m.__doc__ and "VoxelPlane" in m.voxel.__doc__


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # the score chunk is the library's own figure
    chunk = m.voxel.plane_score_chunk()
    assert chunk == lib.mc_voxel_plane_chunk() and 1 <= chunk < 2 ** 20
    assert re.search(rf"constexpr int kPlaneChunk = {chunk};", open(os.path.join(hostbuild.CSRC, "plane.hpp")).read())
    # the library refuses a NULL context itself
    out = (np.zeros(4), np.zeros(3, np.int32), np.zeros(4, np.int64))
    args = (m._lib.ptr(out[0], m._lib.c_double), None, m._lib.ptr(out[1], m._lib.c_int32), m._lib.ptr(out[2], m._lib.c_int64))
    assert lib.mc_voxel_plane(None, 0.1, 10, 0, 1, None, None, *args) == m._lib.MC_ERR_INVALID
    assert out[2].tolist() == [-1, 0, 0, 0] and out[1].tolist() == [-1, -1, -1]
    assert lib.mc_voxel_emit_selected(None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_timing_read_plane(None, None, None) == m._lib.MC_ERR_INVALID
