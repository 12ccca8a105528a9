"""The frames of a batch registered together, without a GPU: (1) the scalar pieces the kernels of csrc/register.hpp
call (csrc/register_core.hpp: the block map, the per-frame padded tree and its levels, the tail tree, the step and the
freeze of an ended frame), run launch by launch by tests/host/register_frames_host.cpp, built with g++ plainly and
under ASan + UBSan: every frame of every case equals tests/registration.py's ``register`` on that frame's rows bit for
bit, the history included; (2) the block map on 300 frames of 7 points; (3) the known answer per frame and its
measurement; (4) the module surface that needs no device."""
import ctypes
import math
import os
import re
import shutil

import numpy as np
import pytest

import hostbuild
import register_frames as RF
import registration as G
from conftest import pkg

ROOT = hostbuild.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("register_frames_host")
    return tmp, [hostbuild.build(tmp, "register_frames_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


def run_host(exe, tmp, c, tol=1e-6):
    """One case through the harness -> (dict of arrays like a VoxelFrameRegistrations, with normals, counts, the
    frame of every first-level block and the iterations the loop ran; the raw bytes)."""
    cl = RF.cloud()
    src, dst = tmp / "in.bin", tmp / "out.bin"
    M, n, F, K = len(cl["keys"]), len(c["src"]), len(c["counts"]), c["max_iterations"]
    log2cap = 6
    while (1 << log2cap) < 2 * M:
        log2cap += 1
    par = np.concatenate([[cl["h"]], cl["origin"], [RF.MAX_DISTANCE, RF.RADIUS, tol, tol]]).astype(np.float64)
    dim = np.array([M, n, F, RF.MAX_NN, K, log2cap], np.int64)
    src.write_bytes(par.tobytes() + dim.tobytes() + np.asarray(c["counts"], np.int64).tobytes()
                    + np.ascontiguousarray(RF.inits_of(c), np.float64).tobytes() + np.ascontiguousarray(cl["keys"], np.int32).tobytes()
                    + np.ascontiguousarray(cl["cent"], np.float64).tobytes() + np.ascontiguousarray(c["src"], np.float64).tobytes())
    hostbuild.run(exe, src, dst)
    raw = dst.read_bytes()
    normals = np.frombuffer(raw, "<f8", 4 * M, 0).reshape(M, 4)
    counts = np.frombuffer(raw, "<i4", M, 32 * M)
    at = 36 * M
    B = int(np.frombuffer(raw, "<i8", 1, at)[0])
    owner = np.frombuffer(raw, "<i4", B, at + 8)
    at += 8 + 4 * B
    stats = np.zeros((F, 4), np.int64)
    T = np.zeros((F, 4, 4))
    for f in range(F):
        stats[f] = np.frombuffer(raw, "<i8", 4, at)
        T[f] = np.frombuffer(raw, "<f8", 16, at + 32).reshape(4, 4)
        at += 160
    history = np.frombuffer(raw, "<f8", F * K * 8, at).reshape(F, K, 8)
    at += F * K * 64
    ran = int(np.frombuffer(raw, "<i8", 1, at)[0])
    assert at + 8 == len(raw) and stats[:, 3].tolist() == list(c["counts"])
    pairs, done = stats[:, 0], stats[:, 1].astype(np.int32)
    last = history[np.arange(F), np.maximum(done - 1, 0), 1]
    fitness = np.array([int(p) / int(m) if m else 0.0 for p, m in zip(pairs, c["counts"])])
    rmse = np.array([math.sqrt(float(s) / int(p)) if p else 0.0 for s, p in zip(last, pairs)])
    return dict(normals=normals, counts=counts, owner=owner, ran=ran, transformations=T, fitness=fitness, inlier_rmse=rmse, pairs=pairs,
                iterations=done, status=stats[:, 2].astype(np.int8), history=history[:, :int(done.max()) if F else 0]), raw


def given_of(got):
    return G.with_normals(RF.cloud(), got["normals"], got["counts"])


def through_both(exes, name, c=None, key=None):
    """The case through both builds: the same bytes, every frame equal to its restatement.  -> (got, want)"""
    tmp, builds = exes
    c = RF.case(name) if c is None else c
    seen = []
    for exe in builds:
        got, raw = run_host(exe, tmp, c)
        seen.append(raw)
        want = RF.expect(key or name, c, given_of(got))
        assert RF.holds(got, c, want, name) is None, RF.holds(got, c, want, name)
    assert seen[0] == seen[1], name
    return got, want


# ---- (1) every frame equals its single-frame restatement ------------------------------------------------------------
@needs_gxx
def test_the_isolated_voxels_leave_the_corner_as_it_is(exes):
    """What the cloud promises: the corner's normals are axes estimated from three neighbours or more, and the six
    isolated voxels have tests/normals.py's counts."""
    tmp, builds = exes
    got, _ = run_host(builds[0], tmp, RF.case("sizes"))
    k = RF.cloud()["n_corner"]
    assert k == 3 * 256 and (got["counts"][:k] >= 3).all() and got["counts"][k:].tolist() == [1, 2, 2, 3, 3, 3]
    axes = np.abs(got["normals"][:k, :3])
    assert ((axes == 0.0) | (axes == 1.0)).all() and (axes.sum(axis=1) == 1.0).all()


@needs_gxx
@pytest.mark.parametrize("name", ["sizes", "400, 0, 881"])
def test_frames_of_every_size_and_an_empty_one(exes, name):
    """Frames of 1, 255, 256, 257 and 1281 points in one batch (one, one, one, two and five of eight first-level
    blocks used; the rest read as the +0.0 the call left), and counts 400, 0, 881 from one pose for all."""
    got, want = through_both(exes, name)
    c = RF.case(name)
    print(name, got["iterations"].tolist(), RF.frame_of(got, 0)["status"], got["pairs"].tolist())
    blocks = [max(256, 1 << (n - 1).bit_length()) // 256 if n else 0 for n in c["counts"]]      # plane_leaves(n) / 256
    assert got["owner"].tolist() == [f for f, k in enumerate(blocks) for _ in range(k)]
    if name == "sizes":
        assert RF.frame_of(got, 0)["status"] == "too_few_pairs" and (got["pairs"][1:] == c["counts"][1:]).all()
    else:
        assert RF.frame_of(got, 1)["status"] == "empty" and want[1] is None


@needs_gxx
@pytest.mark.parametrize("max_iterations", [30, 1, 2])
def test_mixed_endings_in_one_batch(exes, max_iterations):
    """A frame that converges in one iteration, one that needs three, one with five pairs, one on one plane and an
    empty one: each ended frame's pose, history, pairs and iterations are its single-frame restatement's although the
    call ran on for the others; with max_iterations 1 and 2 that ending is among them."""
    name = {30: "mixed endings", 1: "mixed endings, one iteration", 2: "mixed endings, two iterations"}[max_iterations]
    got, want = through_both(exes, name)
    status = [RF.frame_of(got, f)["status"] for f in range(5)]
    print(name, status, got["iterations"].tolist(), got["pairs"].tolist(), "loop ran", got["ran"])
    if max_iterations == 30:
        assert tuple(status) == RF.MIXED and tuple(got["iterations"]) == RF.MIXED_ITERATIONS
        assert got["ran"] == 3                                  # the loop stops when no frame is live
    else:
        assert tuple(status) == ("converged", "max_iterations", "too_few_pairs", "singular", "empty")
        assert tuple(got["iterations"]) == (1, max_iterations, 1, 1, 0) and got["ran"] == max_iterations
    assert got["pairs"][2] == 5 and np.array_equal(got["transformations"][2], np.eye(4))
    assert np.array_equal(G.bits(got["transformations"][3]), G.bits(G.NEARBY_FLAT)) and got["pairs"][3] == 300
    assert np.array_equal(G.bits(got["transformations"][4]), G.bits(G.NEARBY))
    # the frames that ended in the first iteration are what a call of one iteration leaves of them
    one = RF.expect("mixed endings, one iteration", RF.case("mixed endings, one iteration"), given_of(got))
    for f in (0, 2, 3):
        assert G.equal(RF.frame_of(got, f), one[f]), f


@needs_gxx
def test_a_second_level_between_small_frames(exes):
    """65 537 points between frames of 3 and 300 for two iterations: the large frame's 512 first-level partials per sum
    go through a second level of 2 before the tail, the small frames have none (the plain build alone: the restatement
    of 65 537 points is the cost)."""
    tmp, builds = exes
    c = RF.large_between_small()
    got, _ = run_host(builds[0], tmp, c)
    want = RF.expect("large between small", c, given_of(got))
    assert RF.holds(got, c, want) is None, RF.holds(got, c, want)
    assert got["owner"].tolist() == [0] + [1] * 512 + [2] * 2          # 300 points: 512 leaves
    assert got["iterations"].tolist() == [1, 2, 2] and got["pairs"].tolist() == [3, 65537, 300]
    assert [RF.frame_of(got, f)["status"] for f in range(3)] == ["too_few_pairs", "max_iterations", "max_iterations"]


# ---- (2) the block map ---------------------------------------------------------------------------------------------
@needs_gxx
def test_every_block_finds_its_frame(exes):
    """300 frames of 7 points with empty frames before, among (two in a row) and after them: block b belongs to the
    b-th non-empty frame, an empty frame owns no block, and every frame is its restatement."""
    got, want = through_both(exes, "300 frames of 7")
    c = RF.case("300 frames of 7")
    assert len(c["counts"]) == 304 and sum(1 for n in c["counts"] if n == 7) == 300
    full = [f for f, n in enumerate(c["counts"]) if n]
    assert got["owner"].tolist() == full and full[0] == 1 and full[100] == 103 and full[-1] == 302
    assert [RF.frame_of(got, f)["status"] for f in (0, 101, 102, 303)] == ["empty"] * 4
    assert (got["iterations"][full] == 1).all() and (got["pairs"][full] == 7).all()


# ---- (3) the known answer per frame --------------------------------------------------------------------------------
@needs_gxx
def test_known_answers_are_recovered_per_frame(exes):
    """Four frames on the corner's planes, each moved back by its own pose of RF.POSES and held as float32, the values
    a batch can hold: every coordinate is off by float32's rounding (2^-22 at most below 8), which 2000 points average
    down.  Measured here and printed: |T - known| at most 2.19e-10, 1.15e-09, 1.52e-09 and 6.82e-10 in the four frames,
    each converged in 3 iterations with an rmse of 4e-9 (RF.MEASURED: the largest, rounded up).  The bound asserted is four times the measurement, as
    tests/test_registration_cpu.py gives its known answer; the device adds nothing, its result is this one's bits."""
    got, want = through_both(exes, "known answers")
    worst = 0.0
    for f, T in enumerate(RF.POSES):
        w = want[f]
        err = np.abs(w["transformation"] - T).max()
        worst = max(worst, err)
        print(f"frame {f}: {w['status']} after {w['iterations']}, |T - known| {err:.3g}, rmse {w['inlier_rmse']:.3g}, fitness {w['fitness']}")
        assert w["status"] == "converged" and w["fitness"] == 1.0
    print(f"largest |T - known| {worst:.3g}")
    assert worst <= 4 * RF.MEASURED
    assert len({w["transformation"].tobytes() for w in want}) == 4


# ---- (4) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_register_frames", "mc_timing_read_register_frames")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def _batch(m, ctx, counts):
    """A Batch as the checks see it, without a device."""
    b = object.__new__(m.Batch)
    b.ctx, b.counts, b.n_frames, b.n_points = ctx, np.asarray(counts, np.int64), len(counts), int(sum(counts))
    return b


def test_argument_errors_need_no_device():
    m = pkg()
    ctx = _NoDevice()
    cloud = m.VoxelCloud(ctx, 10, 7, 0.05)
    b = _batch(m, ctx, [5, 0, 3])
    for d in (0, 0.0, -0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="max_distance"):
            cloud.register_frames(b, d)
    with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
        cloud.register_frames(b, 0.2001)
    for src in (np.zeros((5, 3)), [b], None):
        with pytest.raises(ValueError, match="takes a Batch"):
            cloud.register_frames(src, 0.1)
    with pytest.raises(ValueError, match="another context"):
        cloud.register_frames(_batch(m, _NoDevice(), [5]), 0.1)
    skew = np.eye(4)
    skew[0, 1] = 2e-6
    not_finite = np.eye(4)
    not_finite[0, 3] = np.nan
    for T in (skew, not_finite, np.eye(3), np.zeros((4, 4)), "x"):
        with pytest.raises(ValueError, match="init"):
            cloud.register_frames(b, 0.1, init=T)
        with pytest.raises(ValueError, match="init of frame 1"):
            cloud.register_frames(b, 0.1, init=[np.eye(4), T, np.eye(4)])
    for k in (2, 4):
        with pytest.raises(ValueError, match=r"one per frame \(3, 4, 4\)"):
            cloud.register_frames(b, 0.1, init=np.tile(np.eye(4), (k, 1, 1)))
    for it in (0, -1, 1.0, "3", None, True, 2 ** 16 + 1):
        with pytest.raises(ValueError, match="max_iterations"):
            cloud.register_frames(b, 0.1, max_iterations=it)
    for tol in (-1e-9, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="tol_rotation"):
            cloud.register_frames(b, 0.1, tol_rotation=tol)
        with pytest.raises(ValueError, match="tol_translation"):
            cloud.register_frames(b, 0.1, tol_translation=tol)
    with pytest.raises(ValueError, match="radius"):
        cloud.register_frames(b, 0.1, normals_radius=0.3)
    with pytest.raises(ValueError, match="max_nn"):
        cloud.register_frames(b, 0.1, max_nn=2)
    # 2^22 history rows pass, one more frame does not
    many = _batch(m, ctx, [1] * 65)
    with pytest.raises(ValueError, match="lower max_iterations"):
        cloud.register_frames(many, 0.1, max_iterations=2 ** 16)
    closed = m.VoxelCloud(ctx, 10, 6, 0.05)      # not the context's live generation: the checks have passed
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.register_frames(_batch(m, ctx, [1] * 64), 0.1, max_iterations=2 ** 16)
    with pytest.raises(ValueError, match="closed or was replaced"):
        closed.register_frames(_batch(m, ctx, [0, 0]), np.float32(0.1), init=np.tile(np.eye(4), (2, 1, 1)), normals_radius=0.2, max_nn=0,
                               tol_rotation=0, tol_translation=0.0)
    assert m.VoxelFrameRegistrations is m.voxel.VoxelFrameRegistrations
    assert m.VoxelFrameRegistrations._fields == ("transformations", "fitness", "inlier_rmse", "pairs", "iterations", "status", "history")
    assert m.voxel.FRAME_REGISTER_STATUS == m.voxel.REGISTER_STATUS + ("empty",) == RF.STATUS
    r = m.VoxelFrameRegistrations(*[None] * 5, np.array([0, 4, 1], np.int8), None)
    assert r.status_names == ("converged", "empty", "max_iterations")
    assert callable(m.VoxelCloud.register_frames) and callable(m.Context.read_timing_register_frames)
    assert "VoxelFrameRegistrations" in m.__doc__ and "VoxelFrameRegistrations" in m.voxel.__doc__


def test_symbols_exported_and_null_arguments_refused():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    par = m._lib.RegisterParams()
    T, hist, stats = np.ones(16), np.zeros(8), np.ones(4, np.int64)
    out = (m._lib.ptr(T, m._lib.c_double), m._lib.ptr(hist, m._lib.c_double), m._lib.ptr(stats, m._lib.c_int64))
    assert lib.mc_voxel_register_frames(None, None, ctypes.byref(par), None, *out) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_register_frames(None, None, None, None, None, None, None) == m._lib.MC_ERR_INVALID
    assert b"NULL" in lib.mc_last_error()
    assert T.all() and stats.all()                # without a batch nobody knows how many rows there are: nothing is written
    assert lib.mc_timing_read_register_frames(None, None, None) == m._lib.MC_ERR_INVALID
