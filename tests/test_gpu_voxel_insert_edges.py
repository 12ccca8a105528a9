"""Growing a voxel cloud on the device where tests/test_gpu_voxel_insert.py stops short (builders and their conditions:
tests/voxelinsertedges.py, asserted in tests/test_voxel_insert_edges_cpu.py): one insert past the rank scan's first
pass into a cloud that has voxels, records past one pass, keys that collide in every table through builds, growths,
re-observations and a merge, the 64-slot table, 910 frames with runs of empty ones as an insert source and the naming of
a refused point among them, random grids, wide rows, a batch with a time column, and what a grown or merged cloud
invalidates and what survives a call that changes nothing.  Every comparison is exact and with the NumPy restatements of
tests/voxelinsert.py, voxel.py and registration.py only."""
import collections
import ctypes

import numpy as np
import pytest

import registration as R
import voxel as V
import voxeledges as E
import voxelinsert as VI
import voxelinsertedges as IE
from test_gpu_voxel_insert import analyses, as_batch, check, emits, empty_cloud, same_emits, same_results, table

pytestmark = pytest.mark.gpu


def state_of(mc, rec, h, origin=V.ZERO):
    """Restatement records (keys, n, S, SI) as the VoxelSums a merge takes."""
    keys, n, S, SI = rec
    return mc.VoxelSums(np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(n, dtype=np.int32),
                        np.ascontiguousarray(np.column_stack([S, SI]), dtype=np.int64), float(h), np.array(origin, np.float64))


# ---- A: more than one scan pass in one call, on a cloud that has voxels ----------------------------------------------
@pytest.mark.parametrize("source", ["rows", "batch"])
@pytest.mark.parametrize("size", E.SCAN_SIZES)
def test_scan_carry_meets_a_base_rank(gpu_ctx, mc, size, source):
    """256, 257 and 513 chunks in one insert into a cloud of 1000 voxels: k_vox_rank<true> adds the cloud's M to ranks
    that hold k_vox_scan's carry between passes; as rows, and as 11 uneven frames of which one is empty."""
    head, call, counts, h = IE.grown_scan_case(size)
    M, grown, want = IE.grown_scan_want(size)
    cloud = mc.voxel_downsample(head, h, context=gpu_ctx)
    try:
        assert cloud.n_voxels == M
        assert cloud.insert(as_batch(gpu_ctx, counts, call) if source == "batch" else call) == grown
        assert cloud.n_voxels == M + grown
        check(cloud, want, (size, source), n_points=len(head) + len(call))
    finally:
        cloud.close()


def test_records_past_one_pass(gpu_ctx, mc):
    """610 308 records, every key six times: 299 workgroups of k_vox_validate<records> add into one 64-bit word, and the
    rank scan takes a second pass; a record of count 0 in the second pass is named by its index and leaves no trace."""
    ctx = gpu_ctx
    head, h, rec = IE.records_case()
    M, grown, want, N = IE.records_want()
    cloud = mc.voxel_downsample(head, h, context=ctx)
    try:
        before = emits(cloud)
        slots = table(ctx)
        with pytest.raises(ValueError, match=rf"record {IE.RECORDS_BAD} "):
            cloud.merge(state_of(mc, IE.refused_records(), h))
        assert cloud.n_voxels == M and cloud.n_points == len(head) and table(ctx) == slots
        same_emits(emits(cloud), before, "a refused record of the second pass")
        assert cloud.merge(state_of(mc, rec, h)) == grown
        got = check(cloud, want, "records past one pass", n_points=N)
        assert int(got["counts"].astype(np.int64).sum()) == cloud.n_points == len(head) + int(rec[1].sum())
    finally:
        cloud.close()


# ---- B: probe chains in a live, growing table ------------------------------------------------------------------------
def run_steps(ctx, mc, steps, done, h, what):
    """The calls of a builder on the device: after every one the cloud is the restatement's (``done``: IE.replay), the
    table is the rule's, and the voxels the call's items do not name are byte for byte what they were.  -> (cloud, the
    emits after every step)"""
    cloud, seen, N = empty_cloud(ctx, h), [], 0
    assert table(ctx) == (0, 0)
    for k, ((kind, rows, counts), (grown, want, at, items)) in enumerate(zip(steps, done)):
        M = cloud.n_voxels
        before = emits(cloud) if M and kind != "build" else {}
        if kind == "build":
            cloud = mc.voxel_downsample(rows, h, context=ctx)
            new = cloud.n_voxels
        elif kind == "records":
            new = cloud.merge(state_of(mc, IE.point_records(rows, h), h))
        else:
            new = cloud.insert(as_batch(ctx, counts, rows) if kind == "batch" else rows)
        N += len(rows)
        assert new == grown and cloud.n_voxels == (0 if kind == "build" else M) + grown, (what, k)
        assert table(ctx) == at, (what, k)
        after = check(cloud, want, (what, k), n_points=N)
        untouched = ~np.isin(V.pack(before["keys"]), items) if before else None
        for f in before:
            assert before[f][untouched].tobytes() == after[f][:M][untouched].tobytes(), (what, k, f)
        seen.append(after)
    return cloud, seen


def test_chains_through_a_live_growing_table(gpu_ctx, mc):
    """6167 keys that start in the last 2^-12 * 96 of every table: a build, three growths that rehash 2048, 2049 and
    6100 colliding keys at once, new keys that walk over the old voxels' slots and wrap to slot 0, every voxel met again
    at exactly half load, and records through the same chains.  Twice the same bytes, whatever the arrival order; and a
    lookup through the final chains finds every voxel."""
    ctx = gpu_ctx
    _, steps = IE.live_chain_case()
    done = IE.replay(steps, IE.CHAIN_H)
    assert tuple(d[2] for d in done) == IE.LIVE_CHAIN_TABLES
    _, first = run_steps(ctx, mc, steps, done, IE.CHAIN_H, "chain")
    cloud, second = run_steps(ctx, mc, steps, done, IE.CHAIN_H, "chain, again")
    for a, b in zip(first, second):
        same_emits(a, b)
    rows = cloud.rows()
    got = cloud.nearest(rows, IE.CHAIN_H / 2)
    assert np.array_equal(got.ids, np.arange(cloud.n_voxels, dtype=np.int32)) and (got.dist2 == 0.0).all()
    ids, d2 = R.nearest(cloud.keys(), rows[:, :3], IE.CHAIN_H, V.ZERO, rows[:, :3], IE.CHAIN_H / 2)
    assert got.ids.dtype == ids.dtype and got.ids.tobytes() == ids.tobytes() and got.dist2.tobytes() == d2.tobytes()


def test_the_minimum_table_under_insert_and_growth(gpu_ctx, mc):
    """From nothing: 32 colliding keys make the 64-slot table, one more grows it to 128, 31 more fill it to exactly
    half load, one more grows it to 256; every chain wraps."""
    _, steps, h = IE.min_table_case()
    steps = [("rows", rows, None) for rows in steps]
    done = IE.replay(steps, h)
    assert tuple(d[2] for d in done) == IE.MIN_TABLES
    cloud, first = run_steps(gpu_ctx, mc, steps, done, h, "64 slots")
    assert cloud.n_voxels == 65
    _, second = run_steps(gpu_ctx, mc, steps, done, h, "64 slots, again")
    for a, b in zip(first, second):
        same_emits(a, b)


# ---- C: runs of empty frames as an insert source, refusal naming -----------------------------------------------------
@pytest.mark.parametrize("one_voxel", [True, False])
def test_frame_runs_as_an_insert_source(gpu_ctx, mc, one_voxel):
    ctx = gpu_ctx
    counts = E.frame_run_counts()
    rows, h = E.frame_run_rows(one_voxel)
    cloud, want = empty_cloud(ctx, h), VI.Cloud(h)
    for c, a, b in IE.frame_halves():
        assert cloud.insert(as_batch(ctx, c, rows[a:b])) == want.insert(rows[a:b])
        check(cloud, want.result(), (one_voxel, a, b), n_points=b)
    check(cloud, V.downsample(rows, h), (one_voxel, "both halves"))
    other = IE.other_points()
    cloud, want = mc.voxel_downsample(other, h, context=ctx), VI.Cloud(h)
    want.insert(other)
    assert cloud.insert(as_batch(ctx, counts, rows)) == want.insert(rows)
    check(cloud, want.result(), (one_voxel, "910 frames into a cloud"), n_points=len(other) + len(rows))


def test_refused_inserts_are_named_among_empty_frames(gpu_ctx, mc):
    """The lowest refused point of an insert at the first and last point of a batch that begins and ends with empty
    frames, in the one-point frame between empty ones and at points 255, 256 and 512 of a frame: by frame and point for
    a batch (vox_points' binary search, the host's frame_of), by row for rows; and nothing is left behind."""
    ctx = gpu_ctx
    counts = E.frame_run_counts()
    good, h = E.frame_run_rows(False)
    other = IE.other_points()
    cloud = mc.voxel_downsample(other, h, context=ctx)
    want = VI.Cloud(h)
    want.insert(other)
    before = check(cloud, want.result(), "built", n_points=len(other))
    slots = table(ctx)
    for what, at, (f, i, dense) in IE.refusal_cases():
        rows = IE.refused_rows(good, at)
        with pytest.raises(V.Refused) as e:
            want.insert(rows)
        assert e.value.index == dense, what
        with pytest.raises(ValueError, match=rf"frame {f}, point {i} "):
            cloud.insert(as_batch(ctx, counts, rows))
        with pytest.raises(ValueError, match=rf"row {dense} "):
            cloud.insert(rows)
        assert cloud.n_voxels == len(want.keys) and cloud.n_points == len(other) and table(ctx) == slots, what
        same_emits(emits(cloud), before, what)
    # and the cloud still takes the batch
    assert cloud.insert(as_batch(ctx, counts, good)) == want.insert(good)
    check(cloud, want.result(), "the good batch after nine refusals", n_points=len(other) + len(good))


# ---- D: grids --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_grid_fuzz_in_parts(gpu_ctx, mc, seed):
    ctx = gpu_ctx
    h, o, rows64, rows32 = E.fuzz_case(seed)
    what = f"fuzz {seed}: h {h}, origin {o}"
    cloud, want, a = empty_cloud(ctx, h, o), VI.Cloud(h, o), 0
    for c in IE.FUZZ_BATCHES:
        part = rows32[a:a + sum(c)]
        a += sum(c)
        assert cloud.insert(as_batch(ctx, c, part)) == want.insert(part), what
        check(cloud, want.result(), (what, "batches", a), n_points=a)
    check(cloud, V.downsample(rows32, h, o), (what, "float32, whole"))
    cloud, want, a = empty_cloud(ctx, h, o), VI.Cloud(h, o), 0
    for part in IE.fuzz_parts(rows64, IE.FUZZ_ROW_CUTS):
        a += len(part)
        assert cloud.insert(part) == want.insert(part), what
        check(cloud, want.result(), (what, "rows", a), n_points=a)
    check(cloud, V.downsample(rows64, h, o), (what, "float64, whole"))
    # the state of the first part into a cloud of the second
    first, second = rows64[:2049], rows64[2049:]
    state = mc.voxel_downsample(first, h, o, context=ctx).state()
    cloud, want = mc.voxel_downsample(second, h, o, context=ctx), VI.Cloud(h, o)
    want.insert(second)
    assert cloud.merge(state) == want.merge(*VI.records_of(V.downsample(first, h, o))), what
    check(cloud, want.result(), (what, "records"), n_points=4096)


# ---- E: layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [6, 7])
def test_wide_rows_as_an_insert_source(gpu_ctx, mc, ld):
    ctx = gpu_ctx
    h, o = IE.WIDE_GRID
    rows = IE.wide_rows(ld)
    four = np.ascontiguousarray(rows[:, :4])
    want = VI.Cloud(h, o)
    want.insert(four[:IE.WIDE_CUT])
    grown = want.insert(four[IE.WIDE_CUT:])
    plain = mc.voxel_downsample(four[:IE.WIDE_CUT], h, o, context=ctx)
    assert plain.insert(four[IE.WIDE_CUT:]) == grown
    narrow = check(plain, want.result(), f"{ld} columns: the same points in four", n_points=len(rows))
    for head in (rows[:IE.WIDE_CUT], four[:IE.WIDE_CUT]):
        cloud = mc.voxel_downsample(head, h, o, context=ctx)
        assert cloud.insert(rows[IE.WIDE_CUT:]) == grown
        same_emits(check(cloud, want.result(), f"rows of {ld} columns", n_points=len(rows)), narrow)
    check(cloud, V.downsample(four, h, o), f"rows of {ld} columns, whole")


def test_a_batch_with_a_time_column_as_an_insert_source(gpu_ctx):
    ctx = gpu_ctx
    rows, times, h = IE.timed_case()
    seen = {}
    for with_time in (True, False):
        cloud, restated, a = empty_cloud(ctx, h), VI.Cloud(h), 0
        for c in IE.TIMED_COUNTS:
            part = rows[a:a + sum(c)]
            b = ctx.batch(c, with_time=with_time)
            b.upload_columns(*[part[:, k].astype(np.float32) for k in range(4)])
            if with_time:
                b.upload_time(times[a:a + sum(c)])
            assert b.with_time == with_time
            a += sum(c)
            assert cloud.insert(b) == restated.insert(part)
            check(cloud, restated.result(), (with_time, a), n_points=a)
        seen[with_time] = check(cloud, V.downsample(rows, h), (with_time, "whole"))
    same_emits(seen[True], seen[False])


# ---- F: what a grown cloud invalidates and what survives -------------------------------------------------------------
Selected = collections.namedtuple("Selected", "cols")
MASK_MESSAGE = r"must be a bool array of shape \({M},\)"


def everything(cloud, src, frames, mask, h):
    """test_gpu_voxel_insert's analyses and the ones it leaves out: one registration per frame, a selection, and a
    plane among a mask."""
    cols = np.stack(cloud.select(mask).download_columns(), axis=1)
    return dict(analyses(cloud, src, h), frames=cloud.register_frames(frames, 2 * h), selected=Selected(cols),
                among=cloud.segment_plane(h, 200, among=mask))


def corner_frames(ctx, src):
    return as_batch(ctx, [400, 0, 600], np.column_stack([src, np.zeros(len(src))]))


def test_every_analysis_after_a_merge(gpu_ctx, mc):
    ctx, h = gpu_ctx, R.H
    rows = R.corner_rows()
    src = R.moved_back(R.corner_source(1000, 3), R.NEARBY)
    frames = corner_frames(ctx, src)
    one_shot = mc.voxel_downsample(rows, h, context=ctx)
    M = one_shot.n_voxels
    mask = IE.corner_mask(M)
    want_cloud = emits(one_shot)
    want = everything(one_shot, src, frames, mask, h)
    assert want["clusters"].n_clusters >= 1 and want["plane"].n_inliers >= 200 and want["register"].pairs > 100
    assert want["among"].n_inliers >= 100 and not (want["among"].inliers & ~mask).any()
    assert want["frames"].status_names[1] == "empty" and (want["frames"].pairs[[0, 2]] > 50).all()
    assert len(want["selected"].cols) == mask.sum()
    states = [mc.voxel_downsample(part, h, context=ctx).state() for part in IE.corner_parts()]
    cloud = empty_cloud(ctx, h)
    sizes = []
    for state in states:
        cloud.merge(state)
        sizes.append(cloud.n_voxels)
        assert len(cloud.normals(2 * h).normals) == cloud.n_voxels      # between the merges: a stale centroid array shows
    assert sizes[0] < sizes[1] < sizes[2] == M
    same_emits(emits(cloud), want_cloud)
    same_results(everything(cloud, src, frames, mask, h), want)
    # a mask of the length before the last merge
    old = IE.corner_mask(sizes[1])
    with pytest.raises(ValueError, match=MASK_MESSAGE.format(M=M)):
        cloud.select(old)
    with pytest.raises(ValueError, match=MASK_MESSAGE.format(M=M)):
        cloud.segment_plane(h, 200, among=old)
    # and the same after inserts: the analyses the insert file leaves out
    cloud = empty_cloud(ctx, h)
    for part in IE.corner_parts():
        before = cloud.n_voxels
        cloud.insert(part)
    same_results(everything(cloud, src, frames, mask, h), want)
    with pytest.raises(ValueError, match=MASK_MESSAGE.format(M=M)):
        cloud.select(IE.corner_mask(before))
    with pytest.raises(ValueError, match=MASK_MESSAGE.format(M=M)):
        cloud.segment_plane(h, 200, among=IE.corner_mask(before))


def cluster_stats(ctx, K):
    """mc_voxel_cluster_stats at the C entry -> (its return value, the bytes it wrote: points, voxels, cell_min, cell_max)."""
    buf = ctx.device_buffer(36 * K)
    try:
        base = buf.ptr.value
        rc = ctx.lib.mc_voxel_cluster_stats(ctx.handle, base + 8 * K, base, base + 12 * K, base + 24 * K)
        return rc, buf.to_host(np.int32, count=9 * K).tobytes()
    finally:
        buf.close()


def stats_bytes(c):
    return c.points.tobytes() + c.voxels.tobytes() + c.cell_min.tobytes() + c.cell_max.tobytes()


def test_a_call_that_changes_nothing_keeps_the_clustering_and_a_real_one_ends_it(gpu_ctx, mc):
    ctx, h, OK, STATE = gpu_ctx, R.H, mc._lib.MC_OK, mc._lib.MC_ERR_STATE
    rows, extra = R.corner_rows(), IE.corner_extra_point()
    whole = mc.voxel_downsample(np.concatenate([rows, extra]), h, context=ctx)
    want_clusters, want_normals = whole.clusters(2 * h, 3), whole.normals(2 * h)
    refused = np.array(rows[:50])
    refused[7, 1] = np.nan

    cloud = mc.voxel_downsample(rows, h, context=ctx)
    first = cloud.clusters(2 * h, 3)
    K = first.n_clusters
    assert K >= 1
    assert cluster_stats(ctx, K) == (OK, stats_bytes(first))
    normals = cloud.normals(2 * h)
    n, bad, bf = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int32(7)

    def unchanged(what):
        assert cluster_stats(ctx, K) == (OK, stats_bytes(first)), what
        same_results(dict(n=cloud.normals(2 * h)), dict(n=normals))

    # empty calls, through the wrapper (which returns early) and at the library itself
    assert cloud.insert(np.zeros((0, 4))) == 0 and cloud.insert(ctx.batch([0, 0])) == 0
    unchanged("empty inserts")
    assert ctx.lib.mc_voxel_insert_f64(ctx.handle, None, 4, 0, ctypes.byref(n), ctypes.byref(bad)) == OK and (n.value, bad.value) == (0, -1)
    empty = ctx.batch([0, 0, 0])
    assert ctx.lib.mc_voxel_insert_batch(ctx.handle, empty.handle, ctypes.byref(n), ctypes.byref(bf), ctypes.byref(bad)) == OK
    assert ctx.lib.mc_voxel_merge_sums(ctx.handle, None, None, None, 0, ctypes.byref(n), ctypes.byref(bad)) == OK
    unchanged("empty calls of the library")
    with pytest.raises(ValueError, match=r"row 7 "):
        cloud.insert(refused)
    with pytest.raises(ValueError, match=r"frame 0, point 7 "):
        cloud.insert(as_batch(ctx, [50], E.f32(refused)))
    unchanged("refused inserts")
    # a real one: the clustering is gone, the normals are the grown cloud's
    assert cloud.insert(extra) == 1
    assert cluster_stats(ctx, K)[0] == STATE
    assert b"mc_voxel_clusters of the live build first" in ctx.lib.mc_last_error()
    grown_normals = cloud.normals(2 * h)
    same_results(dict(n=grown_normals), dict(n=want_normals))
    assert grown_normals.normals[:len(normals.normals)].tobytes() != normals.normals.tobytes()
    assert cluster_stats(ctx, K)[0] == STATE                    # the normals do not bring it back
    again = cloud.clusters(2 * h, 3)
    same_results(dict(c=again), dict(c=want_clusters))
    assert cluster_stats(ctx, again.n_clusters) == (OK, stats_bytes(want_clusters))
    assert stats_bytes(again) != stats_bytes(first)
    # a merge of nothing new but more points ends it as well; the labels stay, the points grow
    assert cloud.merge(cloud.state()) == 0
    assert cluster_stats(ctx, again.n_clusters)[0] == STATE
    doubled = cloud.clusters(2 * h, 3)
    assert doubled.labels.tobytes() == again.labels.tobytes() and np.array_equal(doubled.points, 2 * again.points)
