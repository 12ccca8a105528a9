"""Every frame of a batch registered against the voxel cloud in one call, on the device (VoxelCloud.register_frames;
csrc/register.hpp k_rg_frames_*): row f of the result is bit for bit tests/registration.py's ``register`` on frame f's
rows with the device's own normals, bit for bit ``cloud.register(batch, frame=f, init=init_f)``, and a second call
gives the same bytes.  The cases are tests/register_frames.py's, the ones tests/test_register_frames_cpu.py runs
through the host harness."""
import ctypes

import numpy as np
import pytest

import register_frames as RF
import registration as G
import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def raw(r):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in r)


def shapes_hold(r, F):
    return (r.transformations.shape == (F, 4, 4) and r.transformations.dtype == np.float64 and r.fitness.shape == (F,)
            and r.fitness.dtype == np.float64 and r.inlier_rmse.shape == (F,) and r.inlier_rmse.dtype == np.float64
            and r.pairs.shape == (F,) and r.pairs.dtype == np.int64 and r.iterations.shape == (F,) and r.iterations.dtype == np.int32
            and r.status.shape == (F,) and r.status.dtype == np.int8 and len(r.status_names) == F
            and r.history.shape == (F, int(r.iterations.max()) if F else 0, 8) and r.history.dtype == np.float64)


def cloud_of(m, ctx):
    c = RF.cloud()
    cloud = m.voxel_downsample(c["rows"], c["h"], context=ctx)
    assert np.array_equal(cloud.rows()[:, :3].view(np.uint64), c["cent"].view(np.uint64))
    nrm = cloud.normals(RF.RADIUS, RF.MAX_NN)
    return cloud, G.with_normals(c, nrm.normals, nrm.counts)


def batch_of(ctx, counts, src):
    b = ctx.batch(counts)
    b.upload_columns(*[src[:, k].astype(np.float32) for k in range(3)], np.zeros(len(src), np.float32))
    return b


def check(cloud, given, c, key, singles=None):
    """register_frames of case c against the restatement of every frame, against register(frame=f) of the frames
    `singles` (None: every non-empty one), and against a second call.  -> (the result, the batch, the restatement)"""
    F = len(c["counts"])
    b = batch_of(cloud.ctx, c["counts"], c["src"])
    kw = dict(max_iterations=c["max_iterations"], normals_radius=RF.RADIUS, max_nn=RF.MAX_NN)
    r = cloud.register_frames(b, RF.MAX_DISTANCE, init=c["inits"], **kw)
    want = RF.expect(key, c, given)
    print(f"{key}: {[(s, int(i), int(p)) for s, i, p in zip(r.status_names, r.iterations, r.pairs)][:8]}")
    assert shapes_hold(r, F), key
    assert RF.holds(r, c, want, key) is None, RF.holds(r, c, want, key)
    T = RF.inits_of(c)
    for f in (range(F) if singles is None else singles):
        if c["counts"][f]:
            one = cloud.register(b, RF.MAX_DISTANCE, frame=f, init=T[f], **kw)
            assert G.equal(RF.frame_of(r, f), one._asdict()), (key, f, one.status, r.status_names[f])
    assert raw(cloud.register_frames(b, RF.MAX_DISTANCE, init=c["inits"], **kw)) == raw(r), key
    return r, b, want


@pytest.mark.parametrize("name", list(RF.CASES))
def test_every_case_equals_the_restatement_and_the_single_calls_twice(gpu_ctx, name):
    """Frames of 1, 255, 256, 257 and 1281 points; counts 400, 0, 881 from one pose; the mixed endings (converged in one
    iteration, in three, five pairs, singular, empty) with max_iterations 30, 1 and 2; 300 frames of 7 points among
    empty ones (every 20th against its single call); four known answers."""
    m = pkg()
    cloud, given = cloud_of(m, gpu_ctx)
    c = RF.case(name)
    r, _, want = check(cloud, given, c, name, singles=range(1, 304, 20) if name == "300 frames of 7" else None)
    if name == "mixed endings":
        assert r.status_names == RF.MIXED and tuple(r.iterations) == RF.MIXED_ITERATIONS
        assert r.pairs[2] == 5 and np.array_equal(r.transformations[2], np.eye(4))
        assert np.array_equal(G.bits(r.transformations[3]), G.bits(G.NEARBY_FLAT))
        assert np.array_equal(G.bits(r.transformations[4]), G.bits(G.NEARBY))
    if name.startswith("mixed endings, "):
        k = c["max_iterations"]
        assert r.status_names == ("converged", "max_iterations", "too_few_pairs", "singular", "empty") and tuple(r.iterations) == (1, k, 1, 1, 0)
    if name == "300 frames of 7":
        assert r.status_names.count("empty") == 4 and (r.pairs[np.asarray(c["counts"]) > 0] == 7).all()
    if name == "known answers":
        assert r.status_names == ("converged",) * 4 and (r.fitness == 1.0).all()
        for f, T in enumerate(RF.POSES):
            assert np.abs(r.transformations[f] - T).max() <= 4 * RF.MEASURED      # tests/test_register_frames_cpu.py's measurement


def test_a_second_level_for_the_large_frame_alone(gpu_ctx):
    """65 537 points between frames of 3 and 300, two iterations: the large frame's 512 first-level partials per sum
    take a second level of 2, the small frames none."""
    m = pkg()
    cloud, given = cloud_of(m, gpu_ctx)
    c = RF.large_between_small()
    ctx = gpu_ctx
    ctx.read_timing_register_frames()
    ctx.timing(True)
    try:
        r, _, _ = check(cloud, given, c, "large between small")
    finally:
        ctx.timing(False)
    assert r.iterations.tolist() == [1, 2, 2] and r.pairs.tolist() == [3, 65537, 300]
    assert r.status_names == ("too_few_pairs", "max_iterations", "max_iterations")
    t = ctx.read_timing_register_frames()
    assert t["tree_ms"] > 0 and t["regions"] == 2 * (1 + 3 * 2), t          # two calls: the normals once, then step, tree, solve twice
    ctx.read_timing_register()                                              # the single calls' own


def test_init_as_none_one_matrix_and_one_per_frame(gpu_ctx):
    """Counts that are no multiples of the 256-point column block, so the padded and the dense offsets differ: init
    None, the identity and a stack of identities are the same bytes; one pose for all and a stack of it too; a stack
    of different poses differs from both and is the restatement's."""
    m = pkg()
    cloud, given = cloud_of(m, gpu_ctx)
    c = RF.case("400, 0, 881")
    b = batch_of(gpu_ctx, c["counts"], c["src"])
    assert b.padded_points > b.n_points
    call = lambda init: cloud.register_frames(b, RF.MAX_DISTANCE, init=init, max_iterations=3)
    eye = [raw(call(None)), raw(call(np.eye(4))), raw(call(np.tile(np.eye(4), (3, 1, 1)))), raw(call([np.eye(4)] * 3))]
    assert len(set(eye)) == 1
    near = [raw(call(G.NEARBY)), raw(call(np.tile(G.NEARBY, (3, 1, 1))))]
    assert len(set(near)) == 1 and near[0] != eye[0]
    each = dict(c, inits=np.stack([G.NEARBY, G.NEARBY_FLAT, G.KNOWN]))
    r, _, _ = check(cloud, given, each, "400, 0, 881, a pose each")
    assert raw(r) not in (eye[0], near[0]) and np.array_equal(G.bits(r.transformations[1]), G.bits(G.NEARBY_FLAT))
    with pytest.raises(ValueError, match="init of frame 2"):
        call([np.eye(4), np.eye(4), np.eye(4) * 2])
    empty = gpu_ctx.batch([0, 0])
    r = cloud.register_frames(empty, RF.MAX_DISTANCE, init=G.NEARBY)
    assert shapes_hold(r, 2) and r.status_names == ("empty", "empty") and not r.pairs.any() and not r.iterations.any()
    assert np.array_equal(r.transformations, np.tile(G.NEARBY, (2, 1, 1))) and r.history.shape == (2, 0, 8)


@pytest.mark.parametrize("grid", [g for g in V.ORIGIN_GRIDS if V.ORIGIN_GRIDS[g]["batch"]][:1])
def test_a_grid_off_the_default_origin(gpu_ctx, grid):
    """tests/registration.py's grid case on an origin that is no multiple of h, cloud and source as float32 can hold
    them, the source in frames of 400, 0 and 881 points from NEARBY: every frame is the restatement's and its single
    call's."""
    m = pkg()
    c = G.grid_case(grid, 2.0, "nearby", float32=True)
    assert tuple(c["origin"]) != V.ZERO
    cloud = m.voxel_downsample(c["rows"], c["h"], c["origin"], context=gpu_ctx)
    assert np.array_equal(cloud.keys(), c["keys"])
    nrm = cloud.normals(c["radius"], c["max_nn"])
    given = G.with_normals(c, nrm.normals, nrm.counts)
    counts = [400, 0, 881]
    b = batch_of(gpu_ctx, counts, c["src"])
    kw = dict(init=c["init"], max_iterations=c["max_iterations"], normals_radius=c["radius"], max_nn=c["max_nn"])
    r = cloud.register_frames(b, c["max_distance"], **kw)
    assert shapes_hold(r, 3) and r.status_names[1] == "empty"
    for f, part in ((0, c["src"][:400]), (2, c["src"][400:])):
        want = G.register(given, part, c["max_distance"], init=c["init"], max_iterations=c["max_iterations"])
        got = RF.frame_of(r, f)
        print(f"{grid}, frame {f}: {got['status']} ({want['status']}) after {got['iterations']}, pairs {got['pairs']} ({want['pairs']})")
        assert want["history"][0, 0] >= G.MIN_PAIRS
        assert G.equal(got, want), (grid, f)
        assert G.equal(got, cloud.register(b, c["max_distance"], frame=f, **kw)._asdict()), (grid, f)
    assert raw(cloud.register_frames(b, c["max_distance"], **kw)) == raw(r)


def test_the_loop_closes(gpu_ctx):
    """transform_affine with the result's matrices is the corrected batch: for the four known answers the mean squared
    distance to the nearest centroid is smaller in every frame than before the correction."""
    m = pkg()
    ctx = gpu_ctx
    cloud, _ = cloud_of(m, ctx)
    c = RF.case("known answers")
    b = batch_of(ctx, c["counts"], c["src"])
    r = cloud.register_frames(b, RF.MAX_DISTANCE)
    assert r.status_names == ("converged",) * 4
    before = cloud.nearest(b, RF.MAX_DISTANCE).dist2
    fixed = ctx.transform_affine(b, mats=r.transformations)
    after = cloud.nearest(fixed, RF.MAX_DISTANCE).dist2
    assert np.isfinite(before).all() and np.isfinite(after).all()
    off = np.concatenate([[0], np.cumsum(c["counts"])])
    for f in range(4):
        was, now = before[off[f]:off[f + 1]].mean(), after[off[f]:off[f + 1]].mean()
        print(f"frame {f}: mean dist2 {was:.6g} -> {now:.6g}")
        assert now < was, f


def test_state_lifetime_and_timing(gpu_ctx):
    m = pkg()
    ctx = gpu_ctx
    cloud, given = cloud_of(m, ctx)
    seen = {}
    for name in ("mixed endings", "known answers"):          # five frames and four, three iterations each
        c = RF.case(name)
        b = batch_of(ctx, c["counts"], c["src"])
        ctx.read_timing_register_frames()
        ctx.timing(True)
        try:
            r = cloud.register_frames(b, RF.MAX_DISTANCE, init=c["inits"], max_iterations=c["max_iterations"])
        finally:
            ctx.timing(False)
        t = ctx.read_timing_register_frames()
        assert RF.holds(r, c, RF.expect(name, c, given), name) is None
        assert set(t) == {"normals_ms", "step_ms", "tree_ms", "solve_ms", "regions"}
        assert t["normals_ms"] > 0 and t["step_ms"] > 0 and t["solve_ms"] > 0 and t["tree_ms"] == 0.0, t
        # the launches: a step and a solve per iteration of the loop, and the normals once, however many frames
        assert int(r.iterations.max()) == 3 and t["regions"] - 2 * 3 == 1, t
        seen[name] = t["regions"]
        assert ctx.read_timing_register_frames() == {"normals_ms": 0.0, "step_ms": 0.0, "tree_ms": 0.0, "solve_ms": 0.0, "regions": 0}
    assert seen["mixed endings"] == seen["known answers"] == 7
    # an empty cloud: nobody has a pair
    none = m.voxel_downsample(np.zeros((0, 4)), RF.H, context=ctx)
    r = none.register_frames(b, RF.MAX_DISTANCE)
    assert r.status_names == ("too_few_pairs",) * 4 and not r.pairs.any() and r.iterations.tolist() == [1] * 4
    assert not r.fitness.any() and not r.inlier_rmse.any()
    # a later build on the context ends the cloud; so does close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.register_frames(b, RF.MAX_DISTANCE)
    none.close()
    with pytest.raises(ValueError, match="closed or was replaced"):
        none.register_frames(b, RF.MAX_DISTANCE)


def refused(lib, rc, code, text):
    assert rc == code and lib.mc_last_error().decode() == text, (rc, lib.mc_last_error())


def test_the_library_refuses_in_its_own_words(gpu_ctx):
    """The C entry's refusals after the state lookup and their whole messages, on a context of its own."""
    m = pkg()
    lib, p, cd = m._lib.load(), m._lib.ptr, m._lib.c_double
    INVALID, STATE = m._lib.MC_ERR_INVALID, m._lib.MC_ERR_STATE
    ctx = m.Context(0)
    h = ctx.handle
    c = RF.case("400, 0, 881")
    b = batch_of(ctx, c["counts"], c["src"])
    F = 3

    def tail(max_iterations=2, max_distance=RF.MAX_DISTANCE, frames=F):
        par = m._lib.RegisterParams(max_distance, RF.RADIUS, 1e-6, 1e-6, (ctypes.c_double * 16)(*np.eye(4).reshape(-1).tolist()), 30,
                                    max_iterations)
        out, hist, stats = np.zeros((frames, 16)), np.zeros((frames, min(max_iterations, 4), 8)), np.zeros((frames, 4), np.int64)
        return par, out, stats, (p(out, cd), p(hist, cd), p(stats, m._lib.c_int64))

    par, out, stats, outs = tail()
    refused(lib, lib.mc_voxel_register_frames(h, b.handle, ctypes.byref(par), None, *outs), STATE,
            "mc_voxel_register_frames needs a successful mc_voxel_build_* first")
    assert stats.tolist() == [[0, 0, -1, 0]] * 3 and not out.any()
    cloud = m.voxel_downsample(RF.cloud()["rows"], RF.H, context=ctx)
    assert lib.mc_voxel_register_frames(h, b.handle, ctypes.byref(par), None, *outs) == m._lib.MC_OK
    assert stats[:, 3].tolist() == c["counts"] and stats[:, 2].tolist() == [1, 4, 1] and stats[:, 1].tolist() == [2, 0, 2]
    assert np.array_equal(out[1].reshape(4, 4), np.eye(4))
    # the history cap: 65 frames x 2^16 iterations is one frame over 2^22 rows; nothing is written
    many = ctx.batch([1] * 65)
    par, out, stats, outs = tail(2 ** 16, frames=65)
    refused(lib, lib.mc_voxel_register_frames(h, many.handle, ctypes.byref(par), None, *outs), INVALID,
            "65 frames x max_iterations 65536 is more than 4194304 history rows (256 MB): lower max_iterations")
    other = m.Context(0)
    par, out, stats, outs = tail()
    refused(lib, lib.mc_voxel_register_frames(h, other.batch([4, 4, 4]).handle, ctypes.byref(par), None, *outs), INVALID,
            "batch belongs to another context")
    par, out, stats, outs = tail(max_distance=1.25)
    refused(lib, lib.mc_voxel_register_frames(h, b.handle, ctypes.byref(par), None, *outs), INVALID,
            "max_distance 1.25 is 5 voxels of 0.25 and the search window takes at most 4: voxelise coarser or shrink the radius")
    par, out, stats, outs = tail()
    bad = np.tile(np.eye(4), (3, 1, 1))
    bad[2, 0, 0] = 1.001
    refused(lib, lib.mc_voxel_register_frames(h, b.handle, ctypes.byref(par), p(bad, cd), *outs), INVALID,
            "init of frame 2: the entries must be finite and the rotation orthonormal (|R^T R - I| <= 1e-6)")
    assert lib.mc_voxel_register_frames(h, b.handle, ctypes.byref(par), None, None, outs[1], outs[2]) == INVALID
    assert lib.mc_voxel_register_frames(h, b.handle, None, None, *outs) == INVALID
    cloud.close()
    refused(lib, lib.mc_voxel_register_frames(h, b.handle, ctypes.byref(par), None, *outs), STATE,
            "mc_voxel_register_frames needs a successful mc_voxel_build_* first")
