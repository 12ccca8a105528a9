"""What a batch caches about its columns — the t_ns spans, the evenly-timed rule, the prep key, the PCD text
sums (csrc/batch_state.hpp) — after the writers that tests/test_gpu_time_rule.py's staleness test does
not reach: the LVX, text and LAS decoders, the ray-march scanner's batch emit, the voxel emit and the two
gathers.

Each route runs twice: through its public entry (a new batch), and into an existing batch whose caches a
forgetful writer would leave behind — it holds other points and the other kind of time column (a ramp
where the route writes none, and the reverse), its spans and rule have been read, and two identical
deskews have left tables speculated for a third.  After the write the spans equal NumPy's per-frame
min / max of the downloaded column, the rule equals tests/timerule.py on it, SLERP and IMU deskews are
bit-identical to those of a new batch on a new context filled from the downloaded content, and the text
sums are current exactly for the writers that write them (the scanner's emit).

Frames of 300, 0, 1025 and 1 points: an empty frame, one crossing a 256-point block and a 1024-point
sub-tile, a single point.  (The voxel emit writes one frame of as many points as there are voxels.)
"""
import ctypes
from ctypes import c_double, c_int64

import numpy as np
import pytest

import raymarch as RM
import timerule as TR

pytestmark = pytest.mark.gpu

COUNTS = np.array([300, 0, 1025, 1], np.int64)
OFF = np.concatenate([[0], np.cumsum(COUNTS)])
F, N = len(COUNTS), int(COUNTS.sum())
TICK_NS = 5_000_000                                    # pose and IMU sample spacing
N_TAB = 401                                            # 2 s of table
TIMES = 0.5 + 0.1 * np.arange(F)
STARTS = np.round(TIMES * 1e9).astype(np.int64)
MODES = ("pose_slerp", "imu")


def _tables():
    rng = np.random.default_rng(21)
    time = np.arange(N_TAB) * (TICK_NS * 1e-9)
    pos = np.cumsum(rng.normal(0, 0.05, (N_TAB, 3)), axis=0) + np.array([10.0, -20.0, 2.0])
    rpy = np.column_stack([0.05 * np.sin(1.3 * time), 0.04 * np.cos(0.7 * time), 0.6 * np.sin(0.5 * time)])
    return (time, pos, rpy), (np.arange(N_TAB, dtype=np.int64) * TICK_NS, rng.normal(0, 0.3, (N_TAB, 3)))


TRAJ, IMU = _tables()


def frames_of(counts, fn):
    return np.concatenate([fn(f, int(n)) for f, n in enumerate(counts)] + [np.zeros(0, np.int64)])


def ramp_times(counts=COUNTS):
    """1 us per point from a per-frame t0: evenly timed, inside one table tick or two."""
    return frames_of(counts, lambda f, n: (f + 1) * 777 + 1000 * np.arange(n, dtype=np.int64))


def scattered_times(counts=COUNTS, seed=5):
    """Unsorted times over 50 ms (ten table ticks): no ramp in any frame of three points or more."""
    rng = np.random.default_rng(seed)
    return frames_of(counts, lambda f, n: rng.integers(0, 50_000_000, n))


def rows_of(n, seed):
    """float32-representable x, y, z on a millimetre grid of +-30 m and an integer intensity 0 .. 255."""
    rng = np.random.default_rng(seed)
    a = np.column_stack([rng.integers(-30_000, 30_000, (n, 3)) / 1000.0, rng.integers(0, 256, n)])
    return a.astype(np.float32).astype(np.float64)


def rows5(t_ns, seed=1):
    """(N, 5) file rows: the points and their absolute timestamps (frame start + t_ns)."""
    return np.column_stack([rows_of(N, seed), (np.repeat(STARTS, COUNTS) + t_ns).astype(np.float64)])


def set_tables(ctx):
    ctx.set_trajectory(*TRAJ)
    ctx.set_imu(*IMU)


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    set_tables(gpu_ctx)
    gpu_ctx.time_rule(True)
    return gpu_ctx


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def fresh_deskews(mc, counts, rows, t_ns, times, starts):
    """SLERP and IMU deskews of a new batch on a new context, filled by upload_aos + upload_time: no call
    history, no speculation, no cached spans."""
    c = mc.Context(0)
    set_tables(c)
    b, o = c.batch(counts, with_time=True), c.batch(counts)
    try:
        b.upload_aos(rows)
        b.upload_time(t_ns)
        b.set_frame_times(times)
        b.set_frame_starts(starts)
        return {m: c.deskew(b, o, mode=m).download_aos() for m in MODES}
    finally:
        b.close()
        o.close()
        c.close()


def prime(ctx, b, t_ns, mode, times=TIMES, starts=STARTS):
    """Leave every cache a writer must not forget: other points, the time column t_ns with its spans and
    rule read, text sums that are current, and tables speculated for a third identical call."""
    b.upload_aos(rows_of(b.n_points, 99))
    b.upload_time(t_ns)
    b.set_frame_times(times)
    b.set_frame_starts(starts)
    b.time_spans()
    assert bool(b.time_rule()[0].all()) == bool(np.array_equal(t_ns, ramp_times(b.counts)))
    assert b.pcd_len_current()
    o = ctx.batch(b.counts)
    for _ in range(2):
        ctx.deskew(b, o, mode=mode)
    o.close()


def check(mc, ctx, b, mode, sums, wrote=None, times=TIMES, starts=STARTS):
    """The caches of b against its downloaded content; `mode` is deskewed first (the primed speculation is
    for it).  wrote: the time column the route was given, where the test knows it."""
    counts = b.counts
    off = np.concatenate([[0], np.cumsum(counts)])
    t = b.download_time()
    rows = b.download_aos()
    if wrote is not None:
        assert np.array_equal(t, wrote), "the route did not write the time column it was given"
    lo, hi = b.time_spans()
    even, t0, dt = b.time_rule()
    for f, n in enumerate(counts):
        tf = t[off[f]:off[f + 1]]
        if n:
            assert (lo[f], hi[f]) == (tf.min(), tf.max()), f"span of frame {f}"
        else:
            assert lo[f] > hi[f], f"span of the empty frame {f}"
        assert (bool(even[f]), int(t0[f]), int(dt[f])) == TR.rule_of(tf), f"rule of frame {f}"
    if b.with_pcd_len:
        assert b.pcd_len_current() == sums
    want = fresh_deskews(mc, counts, rows, t, times, starts)
    o = ctx.batch(counts)
    for m in (mode,) + tuple(x for x in MODES if x != mode):
        got = ctx.deskew(b, o, mode=m).download_aos()
        assert np.array_equal(bits(got), bits(want[m])), f"{m} differs from a new batch on a new context"
    o.close()


def target(ctx, counts=COUNTS):
    return ctx.batch(counts, with_time=True, with_pcd_len=True)


def finish_public(b, times=TIMES, starts=STARTS):
    b.set_frame_times(times)
    b.set_frame_starts(starts)
    return b


# ---- (a) the decoders --------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_lvx_decode(mc, ctx, mode):
    """LVX stores no per-point time: the decoder writes the ramp index x point_period_ns."""
    ing, lib, chk, ptr = mc.ingest, ctx.lib, mc._lib.check, mc._lib.ptr
    wrote = frames_of(COUNTS, lambda f, n: 1000 * np.arange(n, dtype=np.int64))
    dev = mc.csim_export.DeviceInfo("3GGDJ6K00200101", 1, "", False, 0, 0, 0, 0, 0, 0)
    data = mc.csim_export.encode_lvx(rows5(wrote), COUNTS, STARTS, None, dev, "lvx2", ctx)
    b, _ = ing.read_lvx_batch(data, point_period_ns=1000, context=ctx)
    assert np.array_equal(b.counts, COUNTS)
    check(mc, ctx, finish_public(b), mode, None, wrote)

    b = target(ctx)
    prime(ctx, b, scattered_times(), mode)
    fmt, pos, slots, _, ts, _ = ing._lvx_index(data)
    d_file, d_tags = ing._upload_file(ctx, data), ctx.device_buffer(N)
    counts = ing._lvx_counts(ctx, fmt, d_file, len(data), pos, slots, False)
    chk(lib.mc_lvx_decode_batch(ctx.handle, fmt, d_file.ptr, len(data), F, ptr(pos, c_int64), ptr(counts, c_int64),
                                ptr(ts, c_int64), 1000, b.handle, d_tags.ptr), "lvx_decode_batch")
    d_file.close()
    d_tags.close()
    check(mc, ctx, b, mode, False, wrote)


@pytest.mark.parametrize("mode", MODES)
def test_text_decode(mc, ctx, mode):
    ing, lib, chk, ptr = mc.ingest, ctx.lib, mc._lib.check, mc._lib.ptr
    wrote = scattered_times()
    body = "".join(f"{r[0]:.3f},{r[1]:.3f},{r[2]:.3f},{r[3]:.1f},{int(r[4])}\n" for r in rows5(wrote)).encode()
    data = ing.CSV_HEADER + b"\n" + body
    b = ing.read_points_batch(data, counts=COUNTS, frame_start_ns=STARTS, context=ctx)
    check(mc, ctx, finish_public(b), mode, None, wrote)

    b = target(ctx)
    prime(ctx, b, ramp_times(), mode)
    d_text = ing._upload_file(ctx, body)
    used, bad = np.zeros(F, np.int64), c_int64()
    chk(lib.mc_text_decode_batch(ctx.handle, ord(","), 5, d_text.ptr, len(body), b.handle, ptr(STARTS, c_int64),
                                 ptr(used, c_int64), ctypes.byref(bad)), "text_decode_batch")
    d_text.close()
    check(mc, ctx, b, mode, False, wrote)


@pytest.mark.parametrize("mode", MODES)
def test_las_decode(mc, ctx, mode):
    lib, chk, ptr = ctx.lib, mc._lib.check, mc._lib.ptr
    wrote = scattered_times()
    data = mc.encode_las(rows5(wrote), "csim", creation_date=(2024, 1), context=ctx)
    b, _ = mc.read_las_batch(data, counts=COUNTS, frame_start_ns=STARTS, context=ctx)
    check(mc, ctx, finish_public(b), mode, None, wrote)

    b = target(ctx)
    prime(ctx, b, ramp_times(), mode)
    h = mc.las._probe(data)
    d_file = mc.ingest._upload_file(ctx, data)
    used, bad = np.zeros(F, np.int64), c_int64(-1)
    chk(lib.mc_las_decode_batch(ctx.handle, d_file.ptr, len(data), h.point_format, h.record_length, h.offset_to_points,
                                h.n_points, ptr(h.scale, c_double), ptr(h.offset, c_double), 1.0, b.handle,
                                ptr(STARTS, c_int64), ptr(used, c_int64), ctypes.byref(bad)), "las_decode_batch")
    d_file.close()
    check(mc, ctx, b, mode, False, wrote)


# ---- (b) the ray-march scanner's batch emit ----------------------------------------------------------------

RAY_CFG = {"points_per_frame": 1120, "fov_horizontal": 1000.0, "range_max": 12.0}   # 16 rings x 70 rays, all kept
RAY_ORIGINS = np.array([[3.0 + f, 400.0 * f, 1.5] for f in range(F)])                # 400 m apart: no cross-talk


def ray_scene():
    """(objects, t_ns): frame f hits exactly COUNTS[f] rays chosen at random — one point per chosen ray on
    the ray, 0.03 past a sample at 7 - 11 m, where neighbouring rays are 0.4 m apart (the hit radius is
    0.1) — so its times, 1000 x ray index, are no ramp."""
    rng = np.random.default_rng(31)
    D, steps = RM.directions(RAY_CFG), RM.steps_of(RAY_CFG)
    assert len(D) == 1120
    objects, t = [], []
    for o, n in zip(RAY_ORIGINS, COUNTS):
        sel = np.sort(rng.choice(len(D), int(n), replace=False))
        pts = o + D[sel] * (steps[rng.integers(70, 110, int(n))] + 0.03)[:, None]
        objects.append(rng.permutation(np.column_stack([pts, rng.uniform(0, 255, int(n))])))
        t.append(1000 * sel)
    return objects, np.concatenate(t)


@pytest.mark.parametrize("mode", MODES)
def test_ray_emit(mc, ctx, mode):
    objects, wrote = ray_scene()
    ori = np.zeros((F, 3))
    sim = mc.LiDARSimulator(dict(RAY_CFG), context=ctx)
    b, _ = sim.scan_frames(RAY_ORIGINS, ori, objects, STARTS, with_pcd_len=True)
    assert np.array_equal(b.counts, COUNTS)
    check(mc, ctx, finish_public(b), mode, True, wrote)

    b = target(ctx)
    prime(ctx, b, ramp_times(), mode)
    counts, _, Rinv = RM.abi_count(mc, ctx, RAY_CFG, RAY_ORIGINS, ori, objects)
    assert np.array_equal(counts, COUNTS)
    mc._lib.check(ctx.lib.mc_ray_emit(ctx.handle, b.handle, RM.ptr(Rinv, c_double), None), "ray_emit")
    check(mc, ctx, b, mode, True, wrote)


# ---- (c) the voxel emit --------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_voxel_emit(mc, ctx, mode):
    """VoxelCloud.batch() makes a batch without a time column: its sums are stale and a frame-mode deskew of
    it equals that of a new batch.  Into a one-frame batch with time the emit leaves the time column alone
    and recomputes its spans."""
    src = ctx.batch(COUNTS)
    src.upload_aos(rows_of(N, 7))
    cloud = ctx.voxel_downsample(src, 2.0)
    M = cloud.n_voxels
    assert 1024 < M <= N, "the voxel points should cross a 1024-point sub-tile"
    b = cloud.batch(with_pcd_len=True)
    assert not b.pcd_len_current()
    b.set_frame_times(TIMES[:1])
    other = mc.Context(0)
    set_tables(other)
    nb = other.batch([M])
    nb.upload_aos(b.download_aos())
    nb.set_frame_times(TIMES[:1])
    want = other.deskew(nb, mode="frame").download_aos()
    nb.close()
    other.close()
    assert np.array_equal(bits(ctx.deskew(b, mode="frame").download_aos()), bits(want))

    one = np.array([M], np.int64)
    t = scattered_times(one)
    b = target(ctx, one)
    prime(ctx, b, t, mode, TIMES[:1], STARTS[:1])
    mc._lib.check(ctx.lib.mc_voxel_emit_batch(ctx.handle, b.handle), "voxel_emit_batch")
    assert np.array_equal(bits(b.download_aos()), bits(cloud.batch().download_aos()))
    check(mc, ctx, b, mode, False, t, TIMES[:1], STARTS[:1])


# ---- (d) the gathers -------------------------------------------------------------------------------------------

def shard(ctx, counts, rows, t_ns):
    b = ctx.batch(counts, with_time=True)
    b.upload_aos(rows)
    b.upload_time(t_ns)
    return b


@pytest.mark.parametrize("mode", MODES)
def test_gather_batches(mc, ctx, mode):
    wrote, rows = scattered_times(), rows_of(N, 3)
    k = int(OFF[2])
    shards = [shard(ctx, COUNTS[:2], rows[:k], wrote[:k]), shard(ctx, COUNTS[2:], rows[k:], wrote[k:])]
    for root in (0, 1):
        merged = target(ctx)
        prime(ctx, merged, ramp_times(), mode)
        mc.dist.gather_batches(ctx, shards, root=root, merged=merged)
        assert np.array_equal(merged.download_aos(), rows)
        check(mc, ctx, merged, mode, False, wrote)


@pytest.fixture(scope="module")
def comm(mc, ctx):
    """One single-rank communicator for both cases (RCCL's start-up takes seconds)."""
    c = mc.dist.RcclComm(ctx, mc.dist.Rendezvous(0, 1))
    yield c
    c.close()


@pytest.mark.parametrize("mode", MODES)
def test_comm_gather_batch_single_rank(mc, ctx, comm, mode):
    wrote, rows = scattered_times(seed=6), rows_of(N, 4)
    local = shard(ctx, COUNTS, rows, wrote)
    merged = target(ctx)
    prime(ctx, merged, ramp_times(), mode)
    comm.gather_batch(local, merged, 0)
    assert np.array_equal(merged.download_aos(), rows)
    check(mc, ctx, merged, mode, False, wrote)
