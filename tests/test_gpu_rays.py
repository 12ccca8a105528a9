"""The rays through a voxel cloud on the device: every count, every `through` and the three stats of VoxelCloud.rays
equal the restatement of tests/rays.py (which tests/test_rays_cpu.py holds to the host build of the core and to exact
arithmetic), the same bytes on a second call; the cloud is left as it was; the counts follow the ids of a cloud that has
grown and shrunk; the ghost is carved out end to end; and the refusals that need a context."""
import ctypes

import numpy as np
import pytest

import rays as R
import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu


def cloud_of(m, ctx, c):
    cloud = m.voxel_downsample(c["rows"], c["h"], c["origin"], context=ctx)
    assert np.array_equal(cloud.keys(), c["keys"])
    return cloud


def raw(r):
    return r.passed.tobytes() + r.ended.tobytes() + r.through.tobytes() + np.array([r.n_rays, r.n_skipped, r.steps]).tobytes()


def holds(r, want, what):
    assert r.passed.dtype == r.ended.dtype == r.through.dtype == np.int32, what
    for k in ("passed", "ended", "through"):
        assert getattr(r, k).tobytes() == want[k].tobytes(), (what, k, getattr(r, k), want[k])
    assert (r.n_rays, r.n_skipped, r.steps) == (want["n_rays"], want["n_skipped"], want["steps"]), what


def state_bytes(cloud):
    s = cloud.state()
    return (s.keys.tobytes(), s.counts.tobytes(), s.sums.tobytes(), np.float64(s.voxel).tobytes(), s.origin.tobytes(), cloud.n_voxels,
            cloud.n_points)


def rays_of_device_origins(m, ctx, cloud, c):
    """mc_voxel_rays_f64 itself, for sensor positions the module refuses (not finite): the library does not read them."""
    rows, o = np.ascontiguousarray(c["src"], np.float64), np.ascontiguousarray(c["origins"], np.float64)
    M, n = cloud.n_voxels, len(rows)
    bufs = [ctx.device_buffer(k) for k in (rows.nbytes, o.nbytes, 4 * M, 4 * M, 4 * n)]
    try:
        bufs[0].from_host(rows)
        bufs[1].from_host(o)
        stats = np.zeros(4, np.int64)
        m._lib.check(ctx.lib.mc_voxel_rays_f64(ctx.handle, bufs[0].ptr, 3, n, bufs[1].ptr, len(o), c["guard"], c["max_steps"],
                                               bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, m._lib.ptr(stats, ctypes.c_int64)), "rays")
        return m.VoxelRays(bufs[2].to_host(np.int32, count=M), bufs[3].to_host(np.int32, count=M), bufs[4].to_host(np.int32, count=n),
                           int(stats[0]), int(stats[1]), int(stats[2]))
    finally:
        for b in bufs:
            b.close()


@pytest.mark.parametrize("name", R.CASES)
def test_case_equals_the_restatement(gpu_ctx, name):
    m, ctx = pkg(), gpu_ctx
    c, want = R.case(name), R.expect(name)
    cloud = cloud_of(m, ctx, c)
    before = state_bytes(cloud)
    if name in R.NOT_FINITE_ORIGINS:
        with pytest.raises(ValueError, match="origins must be finite"):
            cloud.rays(c["src"], c["origins"], guard=c["guard"], max_steps=c["max_steps"])
        call = lambda: rays_of_device_origins(m, ctx, cloud, c)                     # noqa: E731
    else:
        call = lambda: cloud.rays(c["src"], c["origins"], guard=c["guard"], max_steps=c["max_steps"])   # noqa: E731
    first = call()
    holds(first, want, name)
    assert raw(call()) == raw(first), name
    assert state_bytes(cloud) == before, name                                        # the cloud is read, never changed


def test_frames_of_a_batch(gpu_ctx):
    """Frames of 0, 1, 255, 256 and 257 points, one sensor position per frame: the whole batch, every frame alone, one
    position for all frames against (F, 3) of equal rows, and the rows with one position per row."""
    m, ctx = pkg(), gpu_ctx
    c, want = R.case("frames"), R.expect("frames")
    counts, fo = c["counts"], c["frame_origins"]
    cloud = cloud_of(m, ctx, c)
    b = ctx.batch(list(counts))
    b.upload_columns(*[c["src"][:, k].astype(np.float32) for k in range(3)], np.zeros(len(c["src"]), np.float32))
    whole = cloud.rays(b, fo)
    holds(whole, want, "batch")
    assert raw(cloud.rays(c["src"], c["origins"])) == raw(whole)                     # rows, one position per row
    offs = np.concatenate([[0], np.cumsum(counts)])
    for f, n in enumerate(counts):
        if n == 0:
            with pytest.raises(ValueError, match="the source is empty"):
                cloud.rays(b, fo, frame=f)
            continue
        part = c["src"][offs[f]:offs[f + 1]]
        w = R.count(c["keys"], c["h"], c["origin"], part, fo[f], c["guard"], c["max_steps"])
        holds(cloud.rays(b, fo, frame=f), w, f"frame {f}")
        holds(cloud.rays(b, fo[f], frame=f), w, f"frame {f}, its position alone")
    one = cloud.rays(b, fo[2])
    holds(one, R.count(c["keys"], c["h"], c["origin"], c["src"], fo[2], c["guard"], c["max_steps"]), "one position")
    assert raw(cloud.rays(b, np.tile(fo[2], (len(counts), 1)))) == raw(one)
    with pytest.raises(ValueError, match=r"origins must be finite float64 of shape \(3,\) or \(5, 3\), one per frame; got shape \(769, 3\)"):
        cloud.rays(b, c["origins"])
    with pytest.raises(ValueError, match="frame must be an integer in 0..4"):
        cloud.rays(b, fo, frame=5)


def test_counts_follow_a_live_cloud(gpu_ctx):
    """After an insert that grows the table and after a remove that refills it, the counts are those of the cloud's
    current ids: the restatement on the cloud's current keys()."""
    m, ctx = pkg(), gpu_ctx
    c = R.case("frames")
    first = c["rows"][::40]                                                          # 34 voxels: a table of 128 slots
    cloud = m.voxel_downsample(first, c["h"], c["origin"], context=ctx)

    def table():
        slots, growths = ctypes.c_int64(-1), ctypes.c_int64(-1)
        m._lib.check(ctx.lib.mc_voxel_table(ctx.handle, ctypes.byref(slots), ctypes.byref(growths)), "table")
        return slots.value, growths.value

    def check(what):
        keys = cloud.keys()
        r = cloud.rays(c["src"], c["origins"])
        holds(r, R.count(keys, c["h"], c["origin"], c["src"], c["origins"], 1, 4096), what)
        return r

    check("the first cloud")
    slots, growths = table()
    cloud.insert(c["rows"][::-1])                                                    # the box backwards: the ids are not the case's
    assert table()[0] > slots and table()[1] == growths + 1 and cloud.n_voxels == len(c["keys"])
    assert not np.array_equal(cloud.keys(), c["keys"])
    grown = check("after the insert")
    assert sorted(grown.passed.tolist()) == sorted(R.expect("frames")["passed"].tolist())
    rng = np.random.default_rng(3)
    gone = cloud.remove(rng.random(cloud.n_voxels) < 0.5)
    assert 0 < gone < len(c["keys"])
    check("after the remove")
    cloud.remove(np.ones(cloud.n_voxels, bool))                                      # and with nothing left
    r = cloud.rays(c["src"], c["origins"])
    assert len(r.passed) == len(r.ended) == 0 and not r.through.any() and r.steps == R.expect("frames")["steps"]


def test_the_ghost_is_carved_out(gpu_ctx):
    """A wall and a box of points in front of it; the scan sees the wall alone.  remove((passed >= 1) & (ended == 0))
    leaves, bit for bit, the cloud of the wall's points alone."""
    m, ctx = pkg(), gpu_ctx
    c = R.case("ghost")
    cloud = cloud_of(m, ctx, c)
    r = cloud.rays(c["src"], c["origins"], guard=1)
    holds(r, R.expect("ghost"), "ghost")
    mask = (r.passed >= 1) & (r.ended == 0)
    assert cloud.remove(mask) == len(c["box"])
    after = state_bytes(cloud)
    assert after == state_bytes(m.voxel_downsample(c["wall"], c["h"], c["origin"], context=ctx))


def test_refusals_that_need_a_context(gpu_ctx):
    m, ctx = pkg(), gpu_ctx
    c = R.case("axis")
    cloud = cloud_of(m, ctx, c)
    other = m.Context(0)
    b = other.batch([3])
    b.upload_columns(*[c["src"][:, k].astype(np.float32) for k in range(3)], np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="the batch belongs to another context"):
        cloud.rays(b, c["origins"][0])
    m.voxel_downsample(c["rows"][:10], c["h"], c["origin"], context=ctx)
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.rays(c["src"], c["origins"])
