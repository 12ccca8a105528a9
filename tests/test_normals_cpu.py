"""The surface normals of a voxel cloud without a GPU: (1) the scalar core of csrc/normals_core.hpp (on top of
voxel_core.hpp's), included by tests/host/normals_host.cpp, built with
g++ plainly and under ASan + UBSan, and compared with the NumPy restatement of tests/normals.py on every
builder cloud: counts, kept sets and the six covariance values bit for bit, normals and curvature by the
eigenvector criterion; (2) what the builder clouds promise; (3) the module surface that needs no device.

The criterion's constant: the largest (n^T A n - w0) / (2^-52 |A|_F) of the plain g++ build over all builder
clouds is 2.672 (MEASURED_C; reached on the 70 001-voxel slab, 1.44 on the plane and 1.34 on the block; printed
and held below), so the bound is C_BOUND = 4 * 2.672 = 10.688."""
import os
import re
import shutil

import numpy as np
import pytest

import hostbuild
import normals as N
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT
OUT = np.dtype([("n", "<i4"), ("zero", "<i4"), ("C", "<f8", (6,)), ("o", "<f8", (4,)), ("kept", "<u8", (12,))])

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("normals_host")
    return tmp, [hostbuild.build(tmp, "normals_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


def run(exe, tmp, c, viewpoint=None):
    """The harness on a case of tests/normals.py, its table sized as the build sizes it (>= 2 N slots, 64 at least)."""
    keys, cent = c["vox"]["keys"], c["vox"]["rows"][:, :3]
    log2cap = 6
    while (1 << log2cap) < 2 * len(c["rows"]):
        log2cap += 1
    vp = (0.0, 0.0, 0.0) if viewpoint is None else viewpoint
    head = np.array([c["h"], c["radius"], np.float64(c["radius"]) * np.float64(c["radius"]), *vp], np.float64).tobytes()
    dims = np.array([len(keys), c["est"]["R"], c["max_nn"], viewpoint is not None, log2cap], np.int64).tobytes()
    src, dst = tmp / "in.bin", tmp / "out.bin"
    src.write_bytes(head + dims + np.ascontiguousarray(keys, np.int32).tobytes() + np.ascontiguousarray(cent).tobytes())
    hostbuild.run(exe, src, dst)
    return np.frombuffer(dst.read_bytes(), OUT)


def kept_bits(kept):
    """(M, W^3) bool in walk order -> (M, 12) uint64, bit ix of word ix / 64"""
    M, n = kept.shape
    full = np.zeros((M, 768), np.uint8)
    full[:, :n] = kept
    return np.packbits(full, axis=1, bitorder="little").view("<u8")


# ---- (1) the core under g++ ----------------------------------------------------------------------------------
@needs_gxx
def test_core_equals_the_restatement(exes):
    tmp, builds = exes
    worst = {}
    for name in N.CASES:
        c = N.case(name)
        est, cent = c["est"], c["vox"]["rows"][:, :3]
        for b, exe in enumerate(builds):
            for vp in (None, (1000.5, 999.0, 230.0)):
                got = run(exe, tmp, c, vp)
                assert len(got) == len(cent)
                assert np.array_equal(got["kept"], kept_bits(est["kept"])), name
                k = N.check_against(est, got["o"][:, :3], got["o"][:, 3], got["n"], got["C"], vp, cent, name)
                if b == 0 and len(k["rayleigh"]):
                    worst[name] = max(worst.get(name, 0.0), float(k["rayleigh"].max()))
                    print(f"{name:22s} viewpoint {vp is not None:d}: unit {k['unit'].max():.2f}  rayleigh "
                          f"{k['rayleigh'].max():.3f}  curvature {k['curv'].max():.3f}")
    measured = max(worst.values())
    print(f"largest (n^T A n - w0) / (2^-52 F) of the g++ build: {measured:.3f}; MEASURED_C {N.MEASURED_C}, bound {N.C_BOUND}")
    assert measured <= N.MEASURED_C and N.C_BOUND == 4 * N.MEASURED_C


@needs_gxx
@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_core_on_grids_off_the_default_origin(exes, grid):
    """The core takes keys and centroids: those of V.downsample(rows, h, origin) on every grid of V.ORIGIN_GRIDS, at
    radius 2 h and 4 h, held as above."""
    tmp, builds = exes
    for rel in (2.0, 4.0):
        c = N.grid_case(grid, rel)
        est, cent = c["est"], c["vox"]["rows"][:, :3]
        assert 237 <= len(cent) <= 257 and est["R"] == int(rel)
        for exe in builds:
            got = run(exe, tmp, c)
            assert len(got) == len(cent)
            assert np.array_equal(got["kept"], kept_bits(est["kept"])), (grid, rel)
            N.check_against(est, got["o"][:, :3], got["o"][:, 3], got["n"], got["C"], None, cent, (grid, rel))


@needs_gxx
def test_plane_normals_are_the_plane_s(exes):
    """The analytic normal of z = 0.3 x - 0.2 y + 100, within what the criterion and each voxel's own eigenvalue
    gap imply (tests/normals.py plane_angle_bound); most voxels have a wide gap, so the bound bites."""
    tmp, builds = exes
    c = N.case("plane")
    got = run(builds[0], tmp, c)
    k = N.criterion(got["o"][:, :3], got["o"][:, 3], got["C"], got["n"])
    n = got["o"][k["sel"], :3]
    sine = np.linalg.norm(np.cross(n, N.PLANE_NORMAL), axis=1)
    bound = N.plane_angle_bound(k, c["h"])
    assert (sine <= bound).all(), float((sine / bound).max())
    assert np.median(bound) < 1e-6 and (n @ N.PLANE_NORMAL > 0).all()       # canonical sign: z is the largest component
    print(f"plane: largest sine / bound {float((sine / bound).max()):.3f}, median bound {np.median(bound):.2e}, "
          f"smallest gap {k['gap'].min():.3e}")


# ---- (2) what the builder clouds promise -----------------------------------------------------------------------
def test_builder_clouds_hold_what_they_promise():
    c = N.case("plane")
    assert 1300 < len(c["vox"]["rows"]) < 1700 and N.window_radius(c["radius"], c["h"]) == 2
    assert (c["est"]["counts"] >= 3).mean() > 0.95 and c["est"]["counts"].max() <= 30
    # the dense block: 33 neighbours inside, of which the cap keeps 30 — the 27 nearer and three of the six at
    # exactly two cells, the lowest keys: -x, -y, -z
    for name, inside in (("block", 30), ("block uncapped", 33)):
        b = N.case(name)
        keys = b["vox"]["keys"]
        interior = ((keys >= 2) & (keys <= 5)).all(axis=1)
        assert interior.sum() == 64 and (b["est"]["counts"][interior] == inside).all()
        assert (b["est"]["kept"].sum(axis=1) == b["est"]["counts"]).all()
    b = N.case("block")
    i = int(np.flatnonzero(((b["vox"]["keys"] >= 2) & (b["vox"]["keys"] <= 5)).all(axis=1))[0])
    two = [ix for ix in np.flatnonzero(b["est"]["kept"][i])
           if sorted(abs(d - 2) for d in (ix // 25, (ix // 5) % 5, ix % 5)) == [0, 0, 2]]
    assert sorted(two) == [2 * 5 + 2, 2 * 25 + 2, 2 * 25 + 2 * 5]      # (-2, 0, 0), (0, -2, 0), (0, 0, -2) in walk order
    c = N.case("isolated")
    assert c["est"]["counts"].tolist() == N.ISOLATED_COUNTS and np.array_equal(c["vox"]["keys"], N.ISOLATED_CELLS)
    A = N.matrix(c["est"]["cov"][3:])
    assert (np.linalg.matrix_rank(A) == 1).all() and (A[:, 0, 0] > 0).all()       # three collinear voxels: rank 1
    e = N.case("key ends")
    assert e["est"]["counts"].tolist() == N.key_ends()[3]
    assert e["vox"]["keys"][:, 0].min() == V.KEY_MIN and e["vox"]["keys"][:, 1].max() == V.KEY_END - 1
    # a window key packed without the range check would be the decoy's
    assert N.blind_cell([10, V.KEY_END, -3]) == e["vox"]["keys"][6].tolist()
    assert N.blind_cell([11, V.KEY_MIN - 1, -3]) == e["vox"]["keys"][7].tolist()
    assert N.blind_cell([7, -8, 9]) == [7, -8, 9]
    assert len(N.case("30 voxels")["rows"]) == 30 and len(N.case("70001 voxels")["vox"]["rows"]) == 70001
    assert N.case("R = 1")["est"]["R"] == 1 and N.case("R = 4")["est"]["R"] == 4
    assert (N.case("R = 4")["est"]["kept"].sum(axis=1) > 30).sum() == 0 and (N.case("R = 4")["est"]["counts"] == 30).sum() > 100


# ---- (3) the module surface --------------------------------------------------------------------------------
NEW = ("mc_voxel_normals", "mc_timing_read_normals")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def test_argument_errors_need_no_device():
    m = pkg()
    cloud = m.VoxelCloud(_NoDevice(), 10, 7, 0.05)
    for radius in (0, 0.0, -0.1, float("nan"), float("inf"), "x", None, 0.2005, 1.0):
        with pytest.raises(ValueError):
            cloud.normals(radius)
    with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
        cloud.normals(0.2005)
    for max_nn in (1, 2, -1, 65, 30.0, "30", None, True):
        with pytest.raises(ValueError):
            cloud.normals(0.1, max_nn)
    for vp in ((0, 0), (0, 0, float("nan")), (0, float("inf"), 0), 1.0, "abc", (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            cloud.normals(0.1, viewpoint=vp)
    closed = m.VoxelCloud(_NoDevice(), 10, 6, 0.05)      # not the context's live generation
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.normals(0.1)
    assert m.VoxelNormals is m.voxel.VoxelNormals and m.VoxelNormals._fields == ("normals", "curvature", "counts", "covariance")
    assert callable(m.VoxelCloud.normals) and callable(m.Context.read_timing_normals)
    assert "normals" in m.__doc__ and "read_pointcloud.py:81-84" in m.voxel.__doc__


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert "read_pointcloud.py:81-84" in hdr
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # the library refuses the same arguments itself (no context is needed to be told so)
    assert lib.mc_voxel_normals(None, 0.1, 30, None, None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_timing_read_normals(None, None, None) == m._lib.MC_ERR_INVALID
