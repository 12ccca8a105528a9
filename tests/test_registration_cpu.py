"""The registration of a source against a voxel cloud without a GPU: (1) csrc/register_core.hpp compiles alone behind
the stand-ins; (2) the scalar core, included by tests/host/register_host.cpp, built with g++ plainly and under
ASan + UBSan, against the NumPy restatement of tests/registration.py on every case — ids, d2, the 28 sums, every
iteration's step, the final pose and the status bit for bit; (3) the restatement against code that does not share its
definition: a brute-force nearest neighbour, numpy.linalg.solve, the orthonormality of the update; (4) the known
answer; (5) what the builder clouds promise; (6) the module surface that needs no device.  Under (2) also the grids
off the default origin (tests/voxel.py ORIGIN_GRIDS), the radius edge on each of them, and a mutant core whose skip
forgets the origin: equal to the restatement on every case of the default origin, different on every grid."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hostbuild
import registration as G
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


# ---- (1) the core header on its own --------------------------------------------------------------------------------
@needs_gxx
def test_core_header_is_self_contained(tmp_path):
    """tests/test_core_headers.py's line on register_core.hpp itself."""
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "device_standins.hpp"\n#include "register_core.hpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", hostbuild.CSRC, "-I", hostbuild.HOST,
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(os.path.join(hostbuild.CSRC, "register_core.hpp")).read()
    assert not [i for i in re.findall(r"#include\s+[<\"]([^>\"]+)", text) if "hip" in i.lower()]


# ---- (2) the core under g++ ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("register_host")
    return tmp, [hostbuild.build(tmp, "register_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


def run_host(exe, tmp, c, tol=1e-6):
    """One case through the harness -> (dict like the restatement's, with normals and counts; the raw bytes)."""
    src, dst = tmp / "in.bin", tmp / "out.bin"
    M, n = len(c["keys"]), len(c["src"])
    log2cap = 6
    while (1 << log2cap) < 2 * M:
        log2cap += 1
    init = np.eye(4) if c["init"] is None else np.asarray(c["init"], np.float64)
    par = np.concatenate([[c["h"]], c["origin"], [c["max_distance"], c["radius"], tol, tol], init.reshape(-1)]).astype(np.float64)
    dim = np.array([M, n, c["max_nn"], c["max_iterations"], log2cap], np.int64)
    src.write_bytes(par.tobytes() + dim.tobytes() + np.ascontiguousarray(c["keys"], np.int32).tobytes()
                    + np.ascontiguousarray(c["cent"], np.float64).tobytes() + np.ascontiguousarray(c["src"][:, :3], np.float64).tobytes())
    hostbuild.run(exe, src, dst)
    raw = dst.read_bytes()
    at = 36 * M
    normals = np.frombuffer(raw, "<f8", 4 * M, 0).reshape(M, 4)
    counts = np.frombuffer(raw, "<i4", M, 32 * M)
    stats = np.frombuffer(raw, "<i8", 4, at)
    T = np.frombuffer(raw, "<f8", 16, at + 32).reshape(4, 4)
    at += 160
    rows, sums, ids, d2 = [], [], [], []
    for _ in range(int(stats[1])):
        rows.append(np.frombuffer(raw, "<f8", 8, at))
        sums.append(np.frombuffer(raw, "<f8", 28, at + 64))
        ids.append(np.frombuffer(raw, "<i4", n, at + 288))
        d2.append(np.frombuffer(raw, "<f8", n, at + 288 + 4 * n))
        at += 288 + 12 * n
    assert at == len(raw) and int(stats[3]) == n
    pairs = int(stats[0])
    history = np.array(rows)
    return dict(normals=normals, counts=counts, pairs=pairs, iterations=int(stats[1]), status=G.STATUS[int(stats[2])],
                transformation=T, history=history, sums=sums, ids=ids, dist2=d2, fitness=pairs / n,
                inlier_rmse=math.sqrt(float(history[-1, 1]) / pairs) if pairs else 0.0), raw


@needs_gxx
def test_core_equals_the_restatement_on_every_case(exes):
    tmp, builds = exes
    for name in G.CASES:
        c = G.case(name)
        seen = []
        for exe in builds:
            got, raw = run_host(exe, tmp, c)
            seen.append(raw)
            want = G.expect_case(name, got["normals"], got["counts"])
            assert G.equal(got, want), (name, got["status"], want["status"], got["history"], want["history"])
            for i in range(want["iterations"]):
                assert np.array_equal(got["ids"][i], want["ids"][i]), (name, i)
                assert np.array_equal(G.bits(got["dist2"][i]), G.bits(want["dist2"][i])), (name, i)
                assert np.array_equal(G.bits(got["sums"][i]), G.bits(want["sums"][i])), (name, i)
        assert seen[0] == seen[1], name
        print(f"{name}: {want['status']} after {want['iterations']}, pairs {want['pairs']} of {len(c['src'])}")


def holds(got, want):
    """The harness's result equals the restatement's: every field, and every iteration's ids, d2 and sums bit for bit."""
    return (G.equal(got, want) and all(np.array_equal(got["ids"][i], want["ids"][i])
                                       and np.array_equal(G.bits(got["dist2"][i]), G.bits(want["dist2"][i]))
                                       and np.array_equal(G.bits(got["sums"][i]), G.bits(want["sums"][i]))
                                       for i in range(want["iterations"])))


@needs_gxx
@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_core_on_grids_off_the_default_origin(exes, grid):
    """Every run of G.GRID_RUNS (W = 1, 2, 4; from the identity and from NEARBY) on every grid of V.ORIGIN_GRIDS: the
    restatement's nearest walks every cell of the window, the core's leaves out what RegSkip, from cell faces
    o + k h with o not zero, says cannot win."""
    tmp, builds = exes
    for rel, init in G.GRID_RUNS:
        c = G.grid_case(grid, rel, init)
        assert 237 <= len(c["keys"]) <= 257 and len(c["src"]) == 1281
        seen = []
        for exe in builds:
            got, raw = run_host(exe, tmp, c)
            seen.append(raw)
            want = G.grid_expect(grid, rel, init, got["normals"], got["counts"])
            assert holds(got, want), (grid, rel, init, got["status"], want["status"], got["history"], want["history"])
        assert seen[0] == seen[1], (grid, rel, init)
        found = int((want["ids"][0] >= 0).sum())
        print(f"{grid}, {rel} h, {init}: {want['status']} after {want['iterations']}, pairs {want['pairs']}, found {found} of 1281")
        assert found >= 200 and want["history"][0, 0] >= G.MIN_PAIRS          # the source is on the cloud


@needs_gxx
@pytest.mark.parametrize("grid", list(V.ORIGIN_GRIDS))
def test_the_radius_edge_on_every_grid(exes, grid):
    """G.radius_edges through the core, one run per query and max_distance: at the smallest float64 whose square
    reaches the brute-force nearest centroid's d2 that centroid is taken, by the restatement and by the core; at the
    float64 below neither takes it.  None of the 64 is left out."""
    tmp, builds = exes
    c = dict(G.grid_case(grid), max_iterations=1)
    edges = G.radius_edges(grid)
    assert len(edges) == G.EDGE_QUERIES == 64
    for i, e in enumerate(edges):
        assert e["at"] / c["h"] <= 3.5 < 4
        brute = int(np.argmin(G.d2_of(c["cent"], e["q"][0])))
        assert e["want_at"][0][0] == brute and e["want_under"][0][0] != brute, (grid, i)
        assert G.bits(e["want_at"][1])[0] == G.bits(G.d2_of(c["cent"], e["q"][0])[brute])
        for md, (ids, d2) in ((e["at"], e["want_at"]), (e["under"], e["want_under"])):
            for exe in builds:
                got, _ = run_host(exe, tmp, dict(c, src=e["q"], max_distance=md))
                assert np.array_equal(got["ids"][0], ids), (grid, i, md, got["ids"][0], ids)
                assert np.array_equal(G.bits(got["dist2"][0]), G.bits(d2)), (grid, i, md)


SKIP_FACES = ("const double lo = o[a] + (double)k * h;", "const double hi = o[a] + (double)(k + 1) * h;")


@needs_gxx
def test_a_skip_that_forgets_the_origin_shows_only_off_the_default_origin(tmp_path):
    """The mutant: RegSkip's cell faces computed without o[a].  It equals the restatement on every case of G.CASES,
    which all have the origin (0, 0, 0) — the blind spot the grid cases close — and differs from it on each grid of
    V.ORIGIN_GRIDS, so the grid cases cannot be simplified to ones that would miss it."""
    core = hostbuild.preprocessed("register_host.cpp", "-ffp-contract=off")
    for old in SKIP_FACES:
        assert core.count(old) == 1, old
        core = core.replace(old, old.replace("o[a] + ", ""))
    ii = tmp_path / "skip_without_origin.ii"
    ii.write_text(core)
    mutant = hostbuild.build(tmp_path, ii, "-ffp-contract=off")
    for name in G.CASES:
        c = G.case(name)
        assert c["origin"] == V.ZERO
        got, _ = run_host(mutant, tmp_path, c)
        assert holds(got, G.expect_case(name, got["normals"], got["counts"])), name
    for grid in V.ORIGIN_GRIDS:
        differing = 0
        for rel, init in G.GRID_RUNS:
            c = G.grid_case(grid, rel, init)
            got, _ = run_host(mutant, tmp_path, c)
            want = G.grid_expect(grid, rel, init, got["normals"], got["counts"])
            differing += int((got["ids"][0] != want["ids"][0]).sum())
            assert not holds(got, want), (grid, rel, init)
        print(f"{grid}: the mutant's nearest differs from the restatement's in {differing} of {6 * 1281} ids")


@needs_gxx
def test_the_cases_end_as_they_are_meant_to(exes):
    """What the cases promise, on the restatement (which the test above holds the core to)."""
    tmp, builds = exes

    def want(name):
        got, _ = run_host(builds[0], tmp, G.case(name))
        return G.expect_case(name, got["normals"], got["counts"]), got

    w, _ = want("tie")
    assert w["ids"][0].tolist() == G.TIE_WINNERS and (w["dist2"][0] == 0.0625).all()
    w, _ = want("radius edge")
    assert w["ids"][0].tolist() == [0, 0, 0, 0] and w["dist2"][0].tolist() == [0.5625, 0.5625, 0.5625, 0.015625]
    w, _ = want("radius edge, the float64 below")
    assert w["ids"][0].tolist() == [-1, -1, -1, 0] and np.isinf(w["dist2"][0][:3]).all()
    for name in ("window edges, W = 1", "window edges, W = 4"):
        w, _ = want(name)
        ids, d2 = w["ids"][0], w["dist2"][0]
        assert ids[-4:].tolist() == [-1] * 4 and np.isinf(d2[-4:]).all()
        assert ids[:8].tolist() == list(range(8))                              # beside every voxel: itself, decoys included
        assert (ids[8:-4] >= 0).sum() >= 8 and ((ids >= 0) == np.isfinite(d2)).all()
    w, got = want("few neighbours")
    assert got["counts"].tolist() == [1, 2, 2, 3, 3, 3]
    assert (w["ids"][0] >= 0).all() and w["pairs"] == 5 and w["status"] == "too_few_pairs" and w["iterations"] == 1
    assert np.array_equal(w["transformation"], np.eye(4)) and not w["history"][0, 2:].any()
    w, _ = want("six pairs")
    assert w["history"][0, 0] == 6 and w["status"] != "too_few_pairs"
    w, _ = want("one plane")
    c = G.case("one plane")
    assert w["status"] == "singular" and w["iterations"] == 1 and w["pairs"] == len(c["src"])
    assert np.array_equal(G.bits(w["transformation"]), G.bits(c["init"])) and not w["history"][0, 2:].any()
    w, _ = want("known answer, one iteration")
    assert w["status"] == "max_iterations" and w["iterations"] == 1
    w, _ = want("known answer from the answer")
    assert w["status"] == "converged" and w["iterations"] == 1


# ---- (3) the restatement against code that does not share its definition ------------------------------------------
def test_nearest_agrees_with_brute_force():
    """np.argmin over all centroids of |c - q|^2 as one expression, compared where the nearest is unique by a margin
    far above the rounding of either form (1e-9 of r2)."""
    for name in ("slab 1281", "slab 257, W = 1", "slab 257, W = 4", "known answer"):
        c = G.case(name)
        q = G.move(np.eye(4) if c["init"] is None else c["init"], c["src"])
        ids, d2 = G.nearest(c["keys"], c["cent"], c["h"], c["origin"], q, c["max_distance"])
        all_d2 = ((c["cent"][None, :, :] - q[:, None, :]) ** 2).sum(axis=2)
        order = np.argsort(all_d2, axis=1)[:, :2]
        first, second = np.take_along_axis(all_d2, order, axis=1).T
        r2 = c["max_distance"] ** 2
        margin = 1e-9 * r2
        inside = first <= r2 - margin
        outside = first >= r2 + margin
        unique = inside & (second - first > margin)
        assert unique.sum() >= 0.3 * len(q) or name == "slab 257, W = 1", (name, unique.sum())
        assert np.array_equal(ids[unique], order[unique, 0]), name
        assert np.allclose(d2[unique], first[unique], rtol=1e-12, atol=0)
        assert (ids[outside] == -1).all() and np.isinf(d2[outside]).all(), name
        assert outside.any() or name == "known answer", name                   # its source is all within reach


def test_solve_agrees_with_numpy():
    """The Cholesky solve against numpy.linalg.solve on the first iteration's sums of the cases that take a step.
    Both are backward stable: each relative error is at most a small multiple of cond(A) 2^-53; the bound asserted is
    64 cond(A) 2^-53 (6 x 6: the constants of both solvers together), printed beside the figure."""
    rng = np.random.default_rng(3)
    seen = 0
    for name in ("slab 1281", "slab 257, W = 4", "slab 1281 from a pose"):
        c = G.case(name)
        M = len(c["cent"])
        nrm = rng.normal(size=(M, 3))
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        w = G.register(G.with_normals(c, nrm, np.full(M, 3)), c["src"], c["max_distance"], init=c["init"], max_iterations=1)
        s = w["sums"][0]
        x = G.solve(s)
        assert x is not None, name
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = s[:21]
        A = A + np.triu(A, 1).T
        ref = np.linalg.solve(A, -s[21:27])
        cond = np.linalg.cond(A)
        err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
        bound = 64 * cond * 2.0 ** -53
        print(f"{name}: cond(A) {cond:.3g}, relative difference {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, err, bound)
        assert np.array_equal(G.bits(x), G.bits(w["history"][0, 2:]))
        seen += 1
    assert seen == 3
    # a matrix that is not positive definite, and one with a NaN
    s = np.zeros(28)
    s[[0, 6, 11, 15, 18, 20]] = [1, 1, -1e-300, 1, 1, 1]
    assert G.solve(s) is None
    s[11] = np.nan
    assert G.solve(s) is None


def test_update_is_orthonormal():
    rng = np.random.default_rng(4)
    T = np.eye(4)
    worst = 0.0
    for scale in (1e-9, 1e-3, 0.1, 1.0, 10.0):
        for _ in range(20):
            w = rng.normal(size=3) * scale
            D = G.rotation(w)
            worst = max(worst, np.abs(D.T @ D - np.eye(3)).max())
            assert np.linalg.det(D) > 0
            # the rotation vector of dR is w to first order: 2 atan(|w| / 2) about w
            angle = math.acos(min(1.0, max(-1.0, (np.trace(D) - 1) / 2)))
            assert abs(angle - 2 * math.atan(np.linalg.norm(w) / 2)) <= 1e-7
    print(f"|dR^T dR - I| at most {worst:.3g}")
    assert worst <= 8 * 2.0 ** -52
    for _ in range(50):
        T = G.update(T, rng.normal(size=6) * 0.05)
    assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 50 * 8 * 2.0 ** -52


# ---- (4) the known answer ------------------------------------------------------------------------------------------
MEASURED_ROTATION = 1.12e-16       # what the test below prints, rounded up in the third digit
MEASURED_TRANSLATION = 1.39e-17


@needs_gxx
def test_known_answer_is_recovered(exes):
    """The corner cloud's centroids lie exactly on three perpendicular planes and its normals are exactly the axes; the
    source lies on the planes and is moved back by KNOWN (0.03 rad, 0.06 m).  Measured on the restatement with the
    host core's normals (printed below): the largest |R - R_known| entry is 1.11e-16 (MEASURED_ROTATION), the largest
    |t - t_known| entry 1.39e-17 (MEASURED_TRANSLATION), converged in 3 iterations with steps of 6.8e-2, 8.9e-4 and
    4.2e-11 and a residual rmse of 2.4e-11 at the last evaluation.  The bound asserted is four times the measurement: the margin
    for another NumPy build under the source's construction; the device adds none, its result is this one's bits."""
    tmp, builds = exes
    got, _ = run_host(builds[0], tmp, G.case("known answer"))
    assert (got["counts"] >= 3).all()
    axes = np.abs(got["normals"][:, :3])
    assert ((axes == 0.0) | (axes == 1.0)).all() and (axes.sum(axis=1) == 1.0).all()
    w = G.expect_case("known answer", got["normals"], got["counts"])
    dR = np.abs(w["transformation"][:3, :3] - G.KNOWN[:3, :3]).max()
    dt = np.abs(w["transformation"][:3, 3] - G.KNOWN[:3, 3]).max()
    print(f"known answer: {w['status']} after {w['iterations']} iterations, |dR| {dR:.3g}, |dt| {dt:.3g}, "
          f"rmse {w['inlier_rmse']:.3g}, fitness {w['fitness']}, steps {np.linalg.norm(w['history'][:, 2:], axis=1).tolist()}")
    assert w["status"] == "converged" and w["fitness"] == 1.0
    assert dR <= 4 * MEASURED_ROTATION and dt <= 4 * MEASURED_TRANSLATION


# ---- (5) what the builder clouds promise ---------------------------------------------------------------------------
def test_builder_clouds_hold_what_they_promise():
    c = G.corner()
    cent = c["cent"]
    on = [cent[:, 2] == G.H / 2, cent[:, 0] == G.H / 2, cent[:, 1] == G.H / 2]
    assert len(cent) == 3 * 256 and all(m.sum() == 256 for m in on) and (on[0] ^ on[1] ^ on[2]).all()
    assert (c["vox"]["counts"] == 2).all()
    src = G.corner_source(3000, 3000)
    flat = (src == G.H / 2)
    assert (flat.sum(axis=1) == 1).all() and src.min() == G.H / 2 and src.max() < 4.5
    back = G.moved_back(src, G.KNOWN)
    assert np.abs(G.move(G.KNOWN, back) - src).max() <= 8 * np.spacing(4.5)
    R = G.KNOWN[:3, :3]
    assert abs(math.acos((np.trace(R) - 1) / 2) - 0.03) < 2e-3 and abs(np.linalg.norm(G.KNOWN[:3, 3]) - 0.06) < 2e-3
    # the tie's queries are exactly midway on dyadic coordinates, the lower key being the later voxel
    t = G.case("tie")
    for k, w in enumerate(G.TIE_WINNERS):
        a, b = t["cent"][2 * k], t["cent"][2 * k + 1]
        assert np.array_equal((a + b) / 2, t["src"][k]) and V.pack(t["keys"][[w]])[0] < V.pack(t["keys"][[w - 1]])[0]
    e = G.case("radius edge")
    assert e["max_distance"] == G.EDGE_D and np.nextafter(G.case("radius edge, the float64 below")["max_distance"], 1.0) == G.EDGE_D
    assert [len(G.case(f"slab {n}")["src"]) for n in G.SIZES] == list(G.SIZES)


# ---- (6) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_nearest_batch", "mc_voxel_nearest_f64", "mc_voxel_register_batch", "mc_voxel_register_f64",
       "mc_timing_read_register")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def test_argument_errors_need_no_device():
    m = pkg()
    ctx = _NoDevice()
    cloud = m.VoxelCloud(ctx, 10, 7, 0.05)
    rows = np.zeros((5, 3))
    for call in (cloud.nearest, cloud.register):
        for d in (0, 0.0, -0.1, float("nan"), float("inf"), "x", None):
            with pytest.raises(ValueError, match="max_distance"):
                call(rows, d)
        with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
            call(rows, 0.2001)
        for src in (np.zeros((0, 3)), np.zeros((0, 4))):
            with pytest.raises(ValueError, match="empty"):
                call(src, 0.1)
        for src in (np.zeros((5, 2)), np.zeros(5), np.zeros((5, 3, 1))):
            with pytest.raises(ValueError, match="rows must be"):
                call(src, 0.1)
        with pytest.raises(ValueError, match="frame"):
            call(rows, 0.1, frame=0)
    bad_last = np.eye(4)
    bad_last[3, 0] = 1e-3
    skew = np.eye(4)
    skew[0, 1] = 2e-6
    scaled = np.eye(4)
    scaled[:3, :3] *= 1 + 1e-6
    not_finite = np.eye(4)
    not_finite[0, 3] = np.nan
    for T in (bad_last, skew, scaled, not_finite, np.eye(3), np.zeros((4, 4)), "x"):
        with pytest.raises(ValueError, match="transform"):
            cloud.nearest(rows, 0.1, transform=T)
        with pytest.raises(ValueError, match="init"):
            cloud.register(rows, 0.1, init=T)
    for it in (0, -1, 1.0, "3", None, True, 2 ** 16 + 1):
        with pytest.raises(ValueError, match="max_iterations"):
            cloud.register(rows, 0.1, max_iterations=it)
    for tol in (-1e-9, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="tol_rotation"):
            cloud.register(rows, 0.1, tol_rotation=tol)
        with pytest.raises(ValueError, match="tol_translation"):
            cloud.register(rows, 0.1, tol_translation=tol)
    with pytest.raises(ValueError, match="radius"):
        cloud.register(rows, 0.1, normals_radius=0.3)
    with pytest.raises(ValueError, match="max_nn"):
        cloud.register(rows, 0.1, max_nn=2)
    # a pose within the tolerance passes the checks and reaches the liveness test
    nearly = np.eye(4)
    nearly[0, 1] = 5e-7
    closed = m.VoxelCloud(ctx, 10, 6, 0.05)      # not the context's live generation
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.nearest(rows, 0.2, transform=nearly)
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.register(rows, np.float32(0.1), init=nearly, max_iterations=np.int64(2 ** 16), normals_radius=0.2, max_nn=0,
                        tol_rotation=0, tol_translation=0.0)
    assert m.VoxelNearest is m.voxel.VoxelNearest and m.VoxelRegistration is m.voxel.VoxelRegistration
    assert m.VoxelNearest._fields == ("ids", "dist2")
    assert m.VoxelRegistration._fields == ("transformation", "fitness", "inlier_rmse", "pairs", "iterations", "status", "history")
    assert m.voxel.REGISTER_STATUS == G.STATUS
    assert callable(m.VoxelCloud.nearest) and callable(m.VoxelCloud.register) and callable(m.Context.read_timing_register)
    assert "VoxelRegistration" in m.__doc__ and "VoxelRegistration" in m.voxel.__doc__


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # the parameter struct is the header's: four doubles, the pose, two int32
    import ctypes
    assert ctypes.sizeof(m._lib.RegisterParams) == 4 * 8 + 16 * 8 + 2 * 4
    fields = re.search(r"typedef struct mc_register_params \{(.*?)\} mc_register_params;", hdr, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[16\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in m._lib.RegisterParams._fields_], names
    # the library refuses a NULL context itself
    par = m._lib.RegisterParams()
    T, hist, stats = np.ones(16), np.zeros(8), np.ones(4, np.int64)
    out = (m._lib.ptr(T, m._lib.c_double), m._lib.ptr(hist, m._lib.c_double), m._lib.ptr(stats, m._lib.c_int64))
    assert lib.mc_voxel_register_f64(None, None, 3, 1, ctypes.byref(par), *out) == m._lib.MC_ERR_INVALID
    assert stats.tolist() == [0, 0, -1, 0] and not T.any()
    assert lib.mc_voxel_register_batch(None, None, -1, ctypes.byref(par), *out) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_nearest_f64(None, None, 3, 1, 0.1, None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_nearest_batch(None, None, -1, 0.1, None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_timing_read_register(None, None, None) == m._lib.MC_ERR_INVALID
