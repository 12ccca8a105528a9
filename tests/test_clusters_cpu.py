"""The density clustering of a voxel cloud without a GPU: (1) the scalar core of csrc/cluster_core.hpp (on top of
normals_core.hpp's window walker), included by tests/host/cluster_host.cpp, built with g++ plainly and under
ASan + UBSan, run over the voxels forwards, backwards and shuffled — labels, densities and stats byte-equal across
the orders and equal to the NumPy / scipy restatement of tests/clusters.py on every cloud; (2) the same find /
unite text on eight threads under ThreadSanitizer; (3) what the builder clouds promise; (4) a textbook DBSCAN over
scipy's cKDTree on the clouds without exact ties; (5) the module surface that needs no device.

Every output is an integer: all comparisons are exact."""
import os
import re
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest
from scipy.spatial import cKDTree

import clusters as C
import hostbuild
import normals as N
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT
ORDERS = {"forwards": 0, "backwards": 1, "shuffled": 2}

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def write_input(path, c, min_points, weighted, order=0, seed=0):
    """A case of tests/clusters.py as tests/host/cluster_input.hpp reads it, the table sized as the build sizes it."""
    d = c["vox"]
    log2cap = 6
    while (1 << log2cap) < 2 * len(c["rows"]):
        log2cap += 1
    eps = np.float64(c["eps"])
    head = np.array([c["h"], eps, eps * eps], np.float64).tobytes()
    dims = np.array([len(d["keys"]), c["est"]["R"], min_points, weighted, log2cap, order, seed], np.int64).tobytes()
    path.write_bytes(head + dims + np.ascontiguousarray(d["keys"], np.int32).tobytes()
                     + np.ascontiguousarray(d["rows"][:, :3]).tobytes() + np.ascontiguousarray(d["counts"], np.uint32).tobytes())


def read_output(raw, M):
    labels = np.frombuffer(raw, "<i4", M, 0)
    density = np.frombuffer(raw, "<i4", M, 4 * M)
    K = int(np.frombuffer(raw, "<i8", 1, 8 * M)[0])
    at = 8 * M + 8
    voxels = np.frombuffer(raw, "<i4", K, at)
    points = np.frombuffer(raw, "<i8", K, at + 4 * K)
    lo = np.frombuffer(raw, "<i4", 3 * K, at + 12 * K).reshape(K, 3)
    hi = np.frombuffer(raw, "<i4", 3 * K, at + 24 * K).reshape(K, 3)
    assert len(raw) == at + 36 * K
    return dict(labels=labels, density=density, K=K, voxels=voxels, points=points, cell_min=lo, cell_max=hi)


# ---- (1) the core under g++, in three orders ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cluster_host")
    return tmp, [hostbuild.build(tmp, "cluster_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


@needs_gxx
@pytest.mark.parametrize("name", list(C.CASES))
def test_core_equals_the_restatement_in_every_order(exes, name):
    tmp, builds = exes
    c = C.case(name)
    M = len(c["vox"]["keys"])
    src, dst = tmp / "in.bin", tmp / "out.bin"
    for min_points, weighted in c["runs"]:
        want = C.expect(name, min_points, weighted)
        assert C.canonical(want["labels"], want["core"])
        seen = []
        for exe in builds:
            for order in ORDERS.values():
                write_input(src, c, min_points, weighted, order, seed=20261020)
                hostbuild.run(exe, src, dst)
                raw = dst.read_bytes()
                seen.append(raw)
                assert C.equal(read_output(raw, M), want), (name, min_points, weighted, order)
        assert all(raw == seen[0] for raw in seen), (name, min_points, weighted)


@needs_gxx
@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_core_on_grids_off_the_default_origin(exes, grid):
    """The core takes keys, centroids and counts: those of V.downsample(rows, h, origin) on every grid of
    V.ORIGIN_GRIDS, at eps = 2 h, in every order."""
    tmp, builds = exes
    c = C.grid_case(grid)
    M = len(c["vox"]["keys"])
    assert 237 <= M <= 257
    src, dst = tmp / "in.bin", tmp / "out.bin"
    for min_points, weighted in c["runs"]:
        want = C.grid_expect(grid, min_points, weighted)
        assert C.canonical(want["labels"], want["core"])
        seen = []
        for exe in builds:
            for order in ORDERS.values():
                write_input(src, c, min_points, weighted, order, seed=20261020)
                hostbuild.run(exe, src, dst)
                seen.append(dst.read_bytes())
                assert C.equal(read_output(seen[-1], M), want), (grid, min_points, weighted, order)
        assert all(raw == seen[0] for raw in seen), (grid, min_points, weighted)


# ---- (2) find / unite on eight threads under ThreadSanitizer -------------------------------------------------------
@needs_gxx
@pytest.mark.parametrize("name", ["chain", "contention"])
def test_union_find_on_eight_threads_under_tsan(tmp_path_factory, name):
    """The chain is the deep-tree case (ids descend along it), the cube the contended one (six unions per voxel into
    one component).  The harness exits 0 only when every core voxel has the single-threaded run's root and
    parent[x] <= x holds; hostbuild.run refuses any sanitizer report."""
    tmp = tmp_path_factory.mktemp("cluster_tsan_" + name)
    exe = hostbuild.build(tmp, "cluster_tsan_host.cpp", "-ffp-contract=off", "-g", "-fsanitize=thread", "-pthread")
    c = C.case(name)
    (min_points, weighted), = c["runs"]
    for order in ORDERS.values():
        write_input(tmp / "in.bin", c, min_points, weighted, order, seed=8)
        r = hostbuild.run(exe, tmp / "in.bin")
        assert "ThreadSanitizer" not in r.stderr + r.stdout
        assert r.stdout.split() == ["cores", str(len(c["vox"]["keys"])), "differ", "0", "above", "0"], r.stdout


@needs_gxx
def test_core_header_is_self_contained(tmp_path):
    """tests/test_core_headers.py's line on cluster_core.hpp itself."""
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "device_standins.hpp"\n#include "cluster_core.hpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", hostbuild.CSRC, "-I", hostbuild.HOST,
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(os.path.join(hostbuild.CSRC, "cluster_core.hpp")).read()
    assert not [i for i in re.findall(r"#include\s+[<\"]([^>\"]+)", text) if "hip" in i.lower()]


# ---- (3) what the builder clouds promise ---------------------------------------------------------------------------
def summary(e):
    sizes = e["voxels"]
    return dict(K=e["K"], noise=int((e["labels"] < 0).sum()), border=int(((e["labels"] >= 0) & ~e["core"]).sum()),
                largest=int(sizes.max()) if len(sizes) else 0)


def test_builder_clouds_hold_what_they_promise():
    # the tie: the cell between the blocks is not core and both its core neighbours are exactly eps away
    for name, a_number in (("tie", 0), ("tie, B first", 1)):
        c, e = C.case(name), C.expect(name, 4)
        keys = c["vox"]["keys"]
        at = {k: int(np.flatnonzero((keys == k).all(axis=1))[0]) for k in (C.TIE_BETWEEN, (0, 0, 0), (4, 0, 0))}
        between, a0, b0 = at[C.TIE_BETWEEN], at[(0, 0, 0)], at[(4, 0, 0)]
        assert e["density"][between] == 3 and not e["core"][between] and e["core"][a0] and e["core"][b0]
        cent = c["vox"]["rows"][:, :3]
        for other in (a0, b0):
            u = cent[other] - cent[between]
            assert (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2] == 1.0 == np.float64(c["eps"]) * np.float64(c["eps"])
        cores = np.flatnonzero(c["est"]["kept"][between])
        assert sorted(c["est"]["nbr"][between, cores].tolist()) == sorted([between, a0, b0])
        assert e["K"] == 2 and e["labels"][a0] == a_number and e["labels"][b0] == 1 - a_number
        assert e["labels"][between] == a_number                        # A's cell has the lower key
        assert e["density"][e["core"]].min() >= 10 and e["core"].sum() == 36
    # a border voxel that comes before every core of its cluster does not number it: cluster 0 is B's, whose
    # cores appear first, and voxel 0 carries label 1 (numbering by the lowest voxel id would say 0)
    c, e = C.case("tie, border first"), C.expect("tie, border first", 4)
    assert c["vox"]["keys"][0].tolist() == list(C.TIE_BETWEEN) and not e["core"][0] and e["core"][1:].all()
    assert e["labels"][0] == 1 and (e["labels"][1:19] == 0).all() and (e["labels"][19:] == 1).all() and e["K"] == 2
    assert e["voxels"].tolist() == [18, 19]
    # the radius edge
    assert np.array_equal(C.case("isolated")["vox"]["keys"], N.ISOLATED_CELLS)
    assert C.expect("isolated", 3)["labels"].tolist() == [-1, -1, -1, 0, 0, 0]
    assert C.expect("isolated", 2)["labels"].tolist() == [-1, 0, 0, 1, 1, 1]
    under = C.expect("isolated, eps just under", 3)
    assert under["density"].tolist() == [1, 2, 2, 2, 3, 2] and under["labels"].tolist() == [-1, -1, -1, 0, 0, 0]
    assert under["core"].tolist() == [False] * 4 + [True, False]        # a core and two border voxels
    # the chain: ids descend along the path
    c, e = C.case("chain"), C.expect("chain", 2)
    cells = C.chain_cells()
    assert len(np.unique(cells, axis=0)) == 5000 and np.array_equal(c["vox"]["keys"], cells[::-1])
    assert (np.abs(np.diff(cells, axis=0)).sum(axis=1) == 1).all()
    assert summary(e) == dict(K=1, noise=0, border=0, largest=5000) and e["density"].min() == 2 and e["density"].max() == 3
    # contention
    c, e = C.case("contention"), C.expect("contention", 1)
    assert c["est"]["R"] == 1 and summary(e) == dict(K=1, noise=0, border=0, largest=32768)
    inner = ((c["vox"]["keys"] >= 1) & (c["vox"]["keys"] <= 30)).all(axis=1)
    assert (e["density"][inner] == 7).all() and e["density"].min() == 4
    assert summary(C.expect("block", 1))["K"] == 1
    assert summary(C.expect("70001 voxels", 1)) == dict(K=194, noise=0, border=0, largest=69746)
    # the slabs
    assert len(C.case("30 voxels")["rows"]) == 30 and len(C.case("70001 voxels")["vox"]["keys"]) == 70001
    s4, s10 = summary(C.expect("257 voxels", 4)), summary(C.expect("257 voxels", 10))
    assert (s4["K"], s4["noise"], s4["border"]) == (3, 3, 19) and (s10["K"], s10["noise"], s10["border"]) == (6, 126, 95)
    assert summary(C.expect("70001 voxels", 10))["K"] == 1903
    assert C.case("R = 1")["est"]["R"] == 1 and C.case("R = 4")["est"]["R"] == 4
    # the key range's ends: the decoys do not link
    assert summary(C.expect("key ends", 1))["K"] == 4
    e4 = C.expect("key ends", 4)
    assert e4["K"] == 0 and (e4["labels"] == -1).all() and e4["voxels"].shape == (0,) and e4["cell_min"].shape == (0, 3)
    ends = C.expect("key ends", 1)
    assert ends["labels"].tolist() == [0, 0, 0, 1, 1, 1, 2, 3]
    # weighted and unweighted differ in their core sets
    c = C.case("weighted")
    counts = c["vox"]["counts"]
    assert counts.min() == 1 and counts.max() == 6 and len(counts) == 257
    plain, heavy = C.expect("weighted", 10, False), C.expect("weighted", 10, True)
    assert plain["core"].sum() < heavy["core"].sum() < 257 and not np.array_equal(plain["labels"], heavy["labels"])
    assert np.array_equal(plain["density"], C.expect("257 voxels", 10)["density"])
    assert heavy["points"].sum() == counts[heavy["labels"] >= 0].sum()
    for name, mp, w in C.all_runs():
        e = C.expect(name, mp, w)
        assert C.canonical(e["labels"], e["core"]), name


# ---- (4) a textbook DBSCAN over cKDTree ----------------------------------------------------------------------------
def textbook(cent, pairs, eps, min_points):
    """DBSCAN as in the textbook over an undirected edge list: core = at least min_points within eps (itself
    counted), clusters grown breadth-first from the core points in id order through core points; a border point
    goes to the cluster of its nearest core neighbour (no exact ties in these clouds); the rest is noise."""
    M = len(cent)
    adj = [[] for _ in range(M)]
    for a, b in pairs:
        adj[a].append(b)
        adj[b].append(a)
    core = np.array([len(a) + 1 >= min_points for a in adj])
    labels = np.full(M, -1, np.int64)
    K = 0
    for s in range(M):
        if not core[s] or labels[s] >= 0:
            continue
        labels[s] = K
        todo = deque([s])
        while todo:
            a = todo.popleft()
            for b in adj[a]:
                if core[b] and labels[b] < 0:
                    labels[b] = K
                    todo.append(b)
        K += 1
    for v in np.flatnonzero(~core):
        near = [b for b in adj[v] if core[b]]
        if near:
            d = np.linalg.norm(cent[near] - cent[v], axis=1)
            assert len(np.unique(d)) == len(d)
            labels[v] = labels[near[int(np.argmin(d))]]
    return labels, core


@pytest.mark.parametrize("name", ["30 voxels", "257 voxels", "R = 1", "R = 4", "70001 voxels"])
def test_kd_tree_edges_and_a_textbook_dbscan_agree(name):
    """The seeded slabs have no exact ties, so scipy's radius query yields the window walk's edge set and a
    textbook DBSCAN over it the same partition, numbered the same way (both number by the first core voxel)."""
    c = C.case(name)
    cent = c["vox"]["rows"][:, :3]
    pairs = cKDTree(cent).query_pairs(c["eps"], output_type="ndarray")
    i, ix = np.nonzero(c["est"]["kept"])
    j = c["est"]["nbr"][i, ix]
    mine = np.unique(np.stack([i[i < j], j[i < j]], axis=1), axis=0)
    assert np.array_equal(mine, np.unique(np.sort(pairs, axis=1), axis=0))
    if name == "257 voxels":
        assert len(pairs) == 716
    for min_points, weighted in c["runs"]:
        want = C.expect(name, min_points, weighted)
        labels, core = textbook(cent, pairs, c["eps"], min_points)
        assert np.array_equal(core, want["core"]) and np.array_equal(labels, want["labels"]), (name, min_points)


# ---- (5) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_clusters", "mc_voxel_cluster_stats", "mc_timing_read_clusters")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def test_argument_errors_need_no_device():
    m = pkg()
    cloud = m.VoxelCloud(_NoDevice(), 10, 7, 0.05)
    for eps in (0, 0.0, -0.1, float("nan"), float("inf"), "x", None, 0.2005, 1.0):
        with pytest.raises(ValueError):
            cloud.clusters(eps)
    with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
        cloud.clusters(0.2005)
    for min_points in (0, -1, 10.0, 2.5, "10", None, True, False, 2 ** 31):
        with pytest.raises(ValueError, match="min_points"):
            cloud.clusters(0.1, min_points)
    for weighted in (2, -1, 0, 1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="weighted"):
            cloud.clusters(0.1, 10, weighted)
    closed = m.VoxelCloud(_NoDevice(), 10, 6, 0.05)      # not the context's live generation
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.clusters(0.1)
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.clusters(0.1, np.int64(3), weighted=np.True_)
    assert m.VoxelClusters is m.voxel.VoxelClusters
    assert m.VoxelClusters._fields == ("labels", "density", "n_clusters", "voxels", "points", "cell_min", "cell_max")
    assert callable(m.VoxelCloud.clusters) and callable(m.Context.read_timing_clusters)
    assert "VoxelClusters" in m.__doc__ and "VoxelClusters" in m.voxel.__doc__


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # the library refuses a NULL context itself
    assert lib.mc_voxel_clusters(None, 0.1, 10, 0, None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_cluster_stats(None, None, None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_timing_read_clusters(None, None, None) == m._lib.MC_ERR_INVALID
