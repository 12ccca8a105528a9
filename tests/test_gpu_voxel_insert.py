"""Growing a voxel cloud on the device: after any sequence of insert / merge calls the cloud is bit for bit the
restatement of tests/voxelinsert.py, which tests/test_voxel_insert_cpu.py holds to the one-shot restatement of the
concatenated sources.  Every comparison is exact: keys, counts, the raw sums, and the bits of the float64 rows and of
the float32 batch.

Two of the growth cases are sized by the rule itself rather than as first written down: a one-shot build of 1024
points leaves 2048 slots (the power of two >= 2 N), not 4096, so "exactly half load must not grow" runs on 1024 voxels
of two points each (4096 slots) as well as on the literal sequence; and 6000 points into 8192 slots is one doubling
(2 (2049 + 6000) <= 16 384), so a further insert of 30 000 takes the table three doublings on."""
import ctypes
import pickle

import numpy as np
import pytest

import registration as R
import voxel as V
import voxelinsert as VI
from conftest import pkg

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def emits(cloud):
    """Everything the cloud gives out, on the host."""
    b = cloud.batch()
    cols = np.stack(b.download_columns(), axis=1) if cloud.n_voxels else np.zeros((0, 4), np.float32)
    return dict(keys=cloud.keys(), counts=cloud.point_counts(), rows=cloud.rows(), f32=cols, sums=cloud.state().sums)


def same_emits(a, b, what=""):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def check(cloud, want, what, n_points=None):
    """cloud against a restatement's result() (or V.downsample's dict)."""
    got = emits(cloud)
    assert cloud.n_voxels == len(want["rows"]), what
    assert np.array_equal(got["keys"], want["keys"]), what
    assert np.array_equal(got["counts"], want["counts"]), what
    assert np.array_equal(got["sums"], np.column_stack([want["S"], want["SI"]]).reshape(-1, 4)), what
    assert np.array_equal(bits(got["rows"]), bits(want["rows"])), what
    assert np.array_equal(bits(got["f32"]), bits(want["f32"])), what
    if n_points is not None:
        assert cloud.n_points == n_points, what
    return got


def table(ctx):
    slots, growths = ctypes.c_int64(-1), ctypes.c_int64(-1)
    pkg()._lib.check(ctx.lib.mc_voxel_table(ctx.handle, ctypes.byref(slots), ctypes.byref(growths)), "table")
    return slots.value, growths.value


def as_batch(ctx, counts, rows):
    b = ctx.batch(counts)
    if len(rows):
        b.upload_columns(*[rows[:, c].astype(np.float32) for c in range(4)])
    return b


def empty_cloud(ctx, h, origin=V.ZERO):
    return pkg().voxel_downsample(np.zeros((0, 4)), h, origin, context=ctx)


COUNTS = [10000, 10001, 9999, 10003, 9998, 10000, 10000]
_cache = {}


def interleaved(h=0.2, origin=V.ZERO, moved=False, float32=True):
    """The 70 001-point, 7-frame cloud of test_gpu_voxel's test_many_workgroups_with_duplicates_across_frames (about
    9 000 voxels whose points interleave across the frames), on the grid named; nobody writes into it."""
    key = (h, tuple(origin), moved, float32)
    if key not in _cache:
        n = sum(COUNTS)
        rng = np.random.default_rng(3)
        centre = rng.integers(-40, 40, (9000, 3))
        pick = rng.integers(0, 9000, n)
        rows = np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (n, 3))) * h, rng.uniform(0, 1, n)])
        if moved:
            rows[:, :3] += np.asarray(origin, np.float64)
        _cache[key] = f32(rows) if float32 else rows
    return _cache[key]


def split_run(ctx, rows, h, origin, calls, what):
    """calls: (kind, first row, end row) in source order, "batch" ones on frame boundaries.  After every call the cloud
    equals the restatement of the prefix."""
    offs = np.concatenate([[0], np.cumsum(COUNTS)])
    cloud, want = empty_cloud(ctx, h, origin), VI.Cloud(h, origin)
    for kind, a, b in calls:
        part = rows[a:b]
        if kind == "batch":
            f0, f1 = np.searchsorted(offs, a), np.searchsorted(offs, b)
            assert offs[f0] == a and offs[f1] == b
            src = as_batch(ctx, COUNTS[f0:f1], part)
        else:
            src = part
        M = cloud.n_voxels
        grown = want.insert(part)
        assert cloud.insert(src) == grown and cloud.n_voxels == M + grown, (what, kind, a, b)
        check(cloud, want.result(), (what, kind, a, b), n_points=b)
    return cloud, want


def frame_cuts(parts):
    offs = np.concatenate([[0], np.cumsum(COUNTS)])
    at = offs[np.linspace(0, len(COUNTS), parts + 1).round().astype(int)]
    return [("batch", int(a), int(b)) for a, b in zip(at[:-1], at[1:])]


def row_cuts(cuts, n):
    at = [0, *cuts, n]
    return [("rows", a, b) for a, b in zip(at[:-1], at[1:])]


# ---- 1. splits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [2, 3, 7])
def test_batches_cut_at_frame_boundaries(gpu_ctx, parts):
    rows = interleaved()
    _, want = split_run(gpu_ctx, rows, 0.2, V.ZERO, frame_cuts(parts), f"{parts} batches")
    assert 5000 < len(want.keys) <= 9000


def test_rows_cut_around_a_chunk_and_at_the_ends(gpu_ctx):
    rows = interleaved()
    split_run(gpu_ctx, rows, 0.2, V.ZERO, row_cuts([1, 2047, 2048, 2049, 70000], len(rows)), "rows")


def test_a_batch_first_then_rows(gpu_ctx):
    rows = interleaved()
    c3, c5 = sum(COUNTS[:3]), sum(COUNTS[:5])
    split_run(gpu_ctx, rows, 0.2, V.ZERO, [("batch", 0, c3), ("rows", c3, c5), ("batch", c5, len(rows))], "mixed")


def test_one_voxel_inserted_twice_doubles_the_counts(gpu_ctx):
    """Frames of 1, 255, 256, 257, 0 and 1000 points, all inside voxel (0, 0, 0): padding slots are not items."""
    counts = [1, 255, 256, 257, 0, 1000]
    rows = f32(np.random.default_rng(1).uniform(0.05, 0.95, (sum(counts), 4)))
    b = as_batch(gpu_ctx, counts, rows)
    cloud = gpu_ctx.voxel_downsample(b, 1.0)
    want = VI.Cloud(1.0)
    want.insert(rows)
    check(cloud, want.result(), "built", n_points=sum(counts))
    assert cloud.insert(b) == 0 == want.insert(rows)
    got = check(cloud, want.result(), "inserted again", n_points=2 * sum(counts))
    assert got["counts"].tolist() == [2 * sum(counts)] and cloud.n_voxels == 1
    assert cloud.insert(rows) == 0 == want.insert(rows)
    check(cloud, want.result(), "and as rows", n_points=3 * sum(counts))


# ---- 2. growth and stable ids ----------------------------------------------------------------------------------------
def own_voxels(first, n, h=0.25, per=1):
    """n voxels of `per` points each, voxel i at the key test_gpu_voxel's own-voxel case gives index first + i."""
    i = np.repeat(np.arange(first, first + n), per)
    keys = np.stack([i % 13 - 6, (i // 13) % 17 - 8, i // 221 - 4], axis=1)
    rng = np.random.default_rng(first + n)
    return f32(np.column_stack([(keys + rng.uniform(0.1, 0.9, (len(i), 3))) * h, rng.uniform(0, 1, len(i))]))


def grow_step(ctx, cloud, want, rows, slots, growths, what):
    """One insert; the table afterwards has `slots` slots after `growths` growths, and the voxels the insert did not
    touch are bit-identical."""
    before = emits(cloud)
    M = cloud.n_voxels
    assert cloud.insert(rows) == want.insert(rows) == len(rows), what
    assert table(ctx) == (slots, growths), what
    after = check(cloud, want.result(), what)
    for k in before:
        assert before[k].tobytes() == after[k][:M].tobytes(), (what, k)


def test_growth_follows_the_rule_and_ids_are_stable(gpu_ctx):
    m, ctx, h = pkg(), gpu_ctx, 0.25
    # 2048 points of their own voxels: 4096 slots, at half load; one more item grows the table
    rows = own_voxels(0, 2048)
    cloud, want = m.voxel_downsample(rows, h, context=ctx), VI.Cloud(h)
    want.insert(rows)
    assert table(ctx) == (4096, 0)
    grow_step(ctx, cloud, want, own_voxels(2048, 1), 8192, 1, "2048 + 1")
    # the same sequence as written: 1024 points leave 2048 slots, 1024 more need 4096, then exactly half load
    rows = own_voxels(0, 1024)
    cloud, want = m.voxel_downsample(rows, h, context=ctx), VI.Cloud(h)
    want.insert(rows)
    assert table(ctx) == (2048, 0)
    grow_step(ctx, cloud, want, own_voxels(1024, 1024), 4096, 1, "1024 + 1024")
    grow_step(ctx, cloud, want, own_voxels(2048, 1), 8192, 2, "2048 in 4096 slots + 1")
    # exactly half load must not grow: 1024 voxels in 4096 slots (two points each), 1024 more items; then one more does
    rows = own_voxels(0, 1024, per=2)
    cloud, want = m.voxel_downsample(rows, h, context=ctx), VI.Cloud(h)
    want.insert(rows)
    assert table(ctx) == (4096, 0) and cloud.n_voxels == 1024
    grow_step(ctx, cloud, want, own_voxels(1024, 1024), 4096, 0, "M + n = cap / 2")
    grow_step(ctx, cloud, want, own_voxels(2048, 1), 8192, 1, "M + n = cap / 2 + 1")
    grow_step(ctx, cloud, want, own_voxels(2049, 6000), 16384, 2, "6000 more")
    grow_step(ctx, cloud, want, own_voxels(8049, 30000), 131072, 3, "30 000 more: three doublings at once")
    # items that are all voxels of the cloud still count as the worst case, and the result does not depend on it
    again = own_voxels(0, 1024, per=2)
    before = table(ctx)
    assert cloud.insert(again) == 0 == want.insert(again) and table(ctx) == before
    check(cloud, want.result(), "re-observed")


# ---- 3. empty ends ---------------------------------------------------------------------------------------------------
def test_empty_ends(gpu_ctx):
    ctx, h, o = gpu_ctx, 0.3, (0.1, -0.2, 0.05)
    rows = f32(np.random.default_rng(5).normal(0, 3, (3000, 4)))
    rows[:, 3] = np.abs(rows[:, 3])
    cloud, want = empty_cloud(ctx, h, o), VI.Cloud(h, o)
    assert cloud.n_voxels == 0 and cloud.n_points == 0 and table(ctx) == (0, 0)
    for src in (np.zeros((0, 4)), np.zeros((0, 7)), ctx.batch([0]), ctx.batch([0, 0, 0])):
        assert cloud.insert(src) == 0 and cloud.n_voxels == 0 and cloud.n_points == 0 and table(ctx) == (0, 0)
    assert cloud.merge(cloud.state()) == 0 and cloud.state().keys.shape == (0, 3) and cloud.state().sums.shape == (0, 4)
    assert cloud.insert(as_batch(ctx, [0, 1200, 0], rows[:1200])) == want.insert(rows[:1200])      # allocates the table
    check(cloud, want.result(), "into the cloud of an empty source", n_points=1200)
    before = emits(cloud)
    for src in (np.zeros((0, 4)), ctx.batch([0]), ctx.batch([0, 0])):
        assert cloud.insert(src) == 0
    same_emits(emits(cloud), before)
    assert cloud.insert(rows[1200:]) == want.insert(rows[1200:])
    check(cloud, V.downsample(rows, h, o), "rows into it", n_points=3000)
    # the library itself: an empty call is MC_OK, a call without a live build is MC_ERR_STATE
    m = pkg()
    n, bad = ctypes.c_int64(7), ctypes.c_int64(7)
    assert ctx.lib.mc_voxel_insert_f64(ctx.handle, None, 4, 0, ctypes.byref(n), ctypes.byref(bad)) == 0 and (n.value, bad.value) == (0, -1)
    assert ctx.lib.mc_voxel_merge_sums(ctx.handle, None, None, None, 0, ctypes.byref(n), ctypes.byref(bad)) == 0
    bare = m.Context(0)
    assert bare.lib.mc_voxel_insert_f64(bare.handle, None, 4, 0, ctypes.byref(n), ctypes.byref(bad)) == m._lib.MC_ERR_STATE
    assert bare.lib.mc_voxel_points(bare.handle, ctypes.byref(n)) == m._lib.MC_ERR_STATE
    assert bare.lib.mc_voxel_emit_sums(bare.handle, None) == m._lib.MC_ERR_STATE


# ---- 4. a refused call leaves no trace -------------------------------------------------------------------------------
@pytest.mark.parametrize("what, col, value", [("nan", 1, np.nan), ("key out of range", 0, 3.0e5), ("intensity", 3, 65537.0)])
def test_a_refused_call_leaves_no_trace(gpu_ctx, what, col, value):
    ctx, h = gpu_ctx, 0.2
    rng = np.random.default_rng(11)
    first = f32(np.column_stack([rng.uniform(-4, 4, (5000, 3)), rng.uniform(0, 1, 5000)]))
    counts = [700, 0, 900, 1500]
    second = f32(np.column_stack([rng.uniform(-4, 4, (sum(counts), 3)) + [40.0, 0.0, 0.0], rng.uniform(0, 1, sum(counts))]))
    at = 700 + 5                                           # frame 2, index 5
    bad = second.copy()
    bad[[at, at + 300, sum(counts) - 1], col] = value      # and later ones: the lowest is named
    for source in ("batch", "rows"):
        cloud = pkg().voxel_downsample(first, h, context=ctx)
        want = VI.Cloud(h)
        want.insert(first)
        before = check(cloud, want.result(), what)
        slots = table(ctx)
        with pytest.raises(V.Refused) as e:
            VI.Cloud(h).insert(bad)
        assert e.value.index == at
        with pytest.raises(ValueError, match=r"frame 2, point 5 " if source == "batch" else rf"row {at} "):
            cloud.insert(as_batch(ctx, counts, bad) if source == "batch" else bad)
        assert cloud.n_voxels == len(want.keys) and cloud.n_points == 5000 and table(ctx) == slots
        same_emits(emits(cloud), before, (what, source))
        # exactly the points that preceded the refused one, none of whose voxels the cloud had: a key left behind
        # without a voxel id would be found here and not ranked
        head = second[:at]
        grown = want.insert(head)
        assert len(np.unique(V.pack(V.quantise(head[:, :3], head[:, 3], h, V.ZERO)[0]))) == grown > 500
        assert cloud.insert(as_batch(ctx, [700, 0, 5], head) if source == "batch" else head) == grown
        check(cloud, want.result(), (what, source, "the head"), n_points=5000 + at)


# ---- 5. records ------------------------------------------------------------------------------------------------------
def test_records_out_and_in(gpu_ctx):
    m, ctx, h, o = pkg(), gpu_ctx, 0.2, (0.05, 0.0, -0.1)
    rows = interleaved()
    A, B = rows[:30000], rows[30000:]
    dB = V.downsample(B, h, o)
    stateB = m.voxel_downsample(B, h, o, context=ctx).state()
    assert np.array_equal(stateB.keys, dB["keys"]) and np.array_equal(stateB.counts, dB["counts"])
    assert np.array_equal(stateB.sums, np.column_stack([dB["S"], dB["SI"]])) and stateB.sums.dtype == np.int64
    assert stateB.voxel == h and stateB.origin.tolist() == list(o)
    stateB = pickle.loads(pickle.dumps(stateB))
    # A, then B's records: the cloud of A || B
    cloud = m.voxel_downsample(A, h, o, context=ctx)
    want = VI.Cloud(h, o)
    want.insert(A)
    assert cloud.merge(stateB) == want.merge(*VI.records_of(dB))
    check(cloud, V.downsample(rows, h, o), "A merged with B", n_points=len(rows))
    check(cloud, want.result(), "A merged with B, restated")
    # a state that repeats keys: records are items
    twice = m.VoxelSums(*(np.concatenate([a, a[:4000][::-1]]) for a in stateB[:3]), stateB.voxel, stateB.origin)
    assert cloud.merge(twice) == 0 == want.merge(*(np.concatenate([a, a[:4000][::-1]]) for a in VI.records_of(dB)))
    check(cloud, want.result(), "a state with repeated keys")
    # into an empty cloud: B exactly, repeated keys and all
    cloud, want = empty_cloud(ctx, h, o), VI.Cloud(h, o)
    assert cloud.merge(stateB) == len(dB["keys"])
    check(cloud, dB, "B into an empty cloud", n_points=len(B))
    rev = m.VoxelSums(*(np.concatenate([a[::-1], a]) for a in stateB[:3]), stateB.voxel, stateB.origin)
    cloud = empty_cloud(ctx, h, o)
    assert cloud.merge(rev) == want.merge(*(np.concatenate([a[::-1], a]) for a in VI.records_of(dB))) == len(dB["keys"])
    check(cloud, want.result(), "every key twice, new to the cloud", n_points=2 * len(B))
    # another grid, by one ulp
    before = emits(cloud)
    up = np.nextafter(h, 1.0)
    for s in (stateB._replace(voxel=float(up)), stateB._replace(origin=np.array([np.nextafter(o[0], 1.0), o[1], o[2]])),
              stateB._replace(origin=np.array([o[0], o[1], np.nextafter(o[2], -1.0)]))):
        with pytest.raises(ValueError, match="bit for bit"):
            cloud.merge(s)
    # bad records: the lowest is named, the cloud is unchanged
    for field, at, value in (("counts", 17, 0), ("keys", (23, 1), 1 << 20), ("sums", (9, 2), (int(stateB.counts[9]) << 32) + 1),
                             ("sums", (40, 3), -(int(stateB.counts[40]) << 32) - 1), ("counts", 3, -5)):
        arrays = {f: getattr(stateB, f).copy() for f in ("keys", "counts", "sums")}
        arrays[field][at] = value
        later = (at[0] if isinstance(at, tuple) else at) + 1000
        arrays["counts"][later] = 0
        lowest = at[0] if isinstance(at, tuple) else at
        with pytest.raises(V.Refused) as e:
            VI.Cloud(h, o).merge(arrays["keys"], arrays["counts"].astype(np.int64), arrays["sums"][:, :3], arrays["sums"][:, 3])
        assert e.value.index == lowest
        with pytest.raises(ValueError, match=rf"record {lowest} "):
            cloud.merge(stateB._replace(**arrays))
        assert cloud.n_points == 2 * len(B)
        same_emits(emits(cloud), before, field)


# ---- 6. the 2^31 limit without 2^31 points ---------------------------------------------------------------------------
def test_the_point_limit_and_sums_beyond_2_53(gpu_ctx):
    m, ctx, h, o = pkg(), gpu_ctx, 1.0, V.ZERO
    n = 2 ** 30 - 1
    top = n << 32
    keys = np.array([[0, 0, 0], [1, -1, 2]], np.int32)
    counts = np.array([n, n], np.int32)
    sums = np.array([[top, top - 12345, (1 << 53) + 1, 7 - top], [0, top - 1, top // 3, top]], np.int64)
    state = m.VoxelSums(keys, counts, sums, h, np.zeros(3))
    rec = (keys, counts.astype(np.int64), sums[:, :3], sums[:, 3])
    point = np.array([[0.5, 0.25, 0.75, 1.0]])
    cloud, want = empty_cloud(ctx, h, o), VI.Cloud(h, o)
    assert cloud.merge(state) == want.merge(*rec) == 2
    got = check(cloud, want.result(), "two records", n_points=2 * n)
    assert np.array_equal(bits(got["rows"]), bits(V.finalise(keys, sums[:, :3], sums[:, 3], counts, h, o)))
    # the same again would be 2^32 - 4 points
    with pytest.raises(ValueError):
        want.merge(*rec)
    with pytest.raises(ValueError, match=r"2\^31"):
        cloud.merge(state)
    same_emits(emits(cloud), got)
    # one point fits (N = 2^31 - 1), one more does not, as a point or as a record; the library says so itself
    assert cloud.insert(point) == want.insert(point) == 0
    got = check(cloud, want.result(), "one more point", n_points=2 ** 31 - 1)
    with pytest.raises(ValueError):
        want.insert(point)
    with pytest.raises(ValueError, match=r"2\^31"):
        cloud.insert(point)
    one = m.VoxelSums(keys[:1], np.ones(1, np.int32), np.zeros((1, 4), np.int64), h, np.zeros(3))
    with pytest.raises(ValueError, match=r"2\^31"):
        cloud.merge(one)
    buf = ctx.device_buffer(32)
    buf.from_host(point)
    new, bad = ctypes.c_int64(0), ctypes.c_int64(0)
    assert ctx.lib.mc_voxel_insert_f64(ctx.handle, buf.ptr, 4, 1, ctypes.byref(new), ctypes.byref(bad)) == m._lib.MC_ERR_INVALID
    assert bad.value == -1 and b"2^31" in ctx.lib.mc_last_error()
    assert cloud.n_points == 2 ** 31 - 1
    same_emits(emits(cloud), got)
    # both records in one voxel, one merge at a time: accepted twice, a sum of 2^63 - 2^33, refused the third time
    cloud, want = empty_cloud(ctx, h, o), VI.Cloud(h, o)
    half = m.VoxelSums(keys[:1], counts[:1], sums[:1], h, np.zeros(3))
    for k in range(2):
        assert cloud.merge(half) == want.merge(*(a[:1] for a in rec)) == 1 - k
        got = check(cloud, want.result(), f"one voxel, merge {k}", n_points=(k + 1) * n)
    assert got["sums"][0, 0] == 2 * top and got["counts"].tolist() == [2 * n]
    with pytest.raises(ValueError, match=r"2\^31"):
        cloud.merge(half)
    same_emits(emits(cloud), got)


# ---- 7. the analyses see the grown cloud -----------------------------------------------------------------------------
def analyses(cloud, src, h):
    return dict(normals=cloud.normals(2 * h), clusters=cloud.clusters(2 * h, 3), plane=cloud.segment_plane(h, 200),
                nearest=cloud.nearest(src, 2 * h), register=cloud.register(src, 2 * h))


def same_results(a, b):
    for name in a:
        for field, x, y in zip(a[name]._fields, a[name], b[name]):
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, field)
            else:
                assert type(x) is type(y) and repr(x) == repr(y), (name, field)


def test_the_analyses_see_the_grown_cloud(gpu_ctx):
    m, ctx, h = pkg(), gpu_ctx, R.H
    rows = R.corner_rows()
    src = R.moved_back(R.corner_source(1000, 3), R.NEARBY)
    one_shot = m.voxel_downsample(rows, h, context=ctx)
    want_cloud = emits(one_shot)
    want = analyses(one_shot, src, h)
    assert want["clusters"].n_clusters >= 1 and want["plane"].n_inliers >= 200 and want["register"].pairs > 100
    cuts = [0, 400, 1000, len(rows)]
    cloud = empty_cloud(ctx, h)
    partial = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        cloud.insert(rows[a:b])
        partial.append(cloud.normals(2 * h))        # between the inserts: a stale centroid array would show next time
        assert len(partial[-1].normals) == cloud.n_voxels
    same_emits(emits(cloud), want_cloud)
    got = analyses(cloud, src, h)
    same_results(got, want)
    assert partial[-1].normals.tobytes() == want["normals"].normals.tobytes()
    assert len(partial[0].normals) < len(partial[-1].normals)
    # and after a clustering of the partial cloud, the labels are the grown cloud's
    cloud = m.voxel_downsample(rows[:1000], h, context=ctx)
    cloud.clusters(2 * h, 3)
    cloud.insert(rows[1000:])
    same_results(analyses(cloud, src, h), want)


# ---- 8. grids off the origin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid, kind", [("fractional", "batch"), ("fractional", "rows"), ("far keys", "batch"), ("far keys", "rows"),
                                        ("utm", "rows")])
def test_grids_off_the_origin(gpu_ctx, grid, kind):
    g = V.ORIGIN_GRIDS[grid]
    assert g["batch"] or kind == "rows"
    rows = interleaved(g["h"], g["origin"], g["moved"], float32=g["batch"])
    calls = frame_cuts(3) if kind == "batch" else row_cuts([2049, 40000], len(rows))
    _, want = split_run(gpu_ctx, rows, g["h"], g["origin"], calls, (grid, kind))
    whole = V.downsample(rows, g["h"], g["origin"])
    assert np.array_equal(bits(want.result()["rows"]), bits(whole["rows"])) and len(whole["rows"]) > 5000


def test_the_phases_are_timed(gpu_ctx):
    """mc_timing_read_voxel_insert: the event time of the four phases since the last read, and the timed regions (the
    rank phase is two: before and after the synchronisation that sizes the records)."""
    ctx = gpu_ctx
    rows = interleaved()
    cloud = empty_cloud(ctx, 0.2)
    ctx.read_timing_voxel_insert()
    ctx.read_timing_voxel()
    cloud.insert(rows[:1000])                     # not timed
    assert ctx.read_timing_voxel_insert() == dict(validate_ms=0.0, insert_ms=0.0, rank_ms=0.0, accumulate_ms=0.0, regions=0)
    ctx.timing(True)
    try:
        cloud.insert(rows[1000:30000])
        cloud.merge(cloud.state())
    finally:
        ctx.timing(False)
    t = ctx.read_timing_voxel_insert()
    assert t["regions"] == 10 and all(0.0 < t[k] < 1000.0 for k in ("validate_ms", "insert_ms", "rank_ms", "accumulate_ms")), t
    assert ctx.read_timing_voxel_insert()["regions"] == 0
    assert ctx.read_timing_voxel()["regions"] == 2      # state()'s keys and counts: the filter's finalise phase, another list


# ---- 9. twice the same bits ------------------------------------------------------------------------------------------
def test_twice_the_same_bits_and_the_one_shot_build_after(gpu_ctx):
    ctx = gpu_ctx
    rows = interleaved()
    seen = []
    for _ in range(2):
        cloud, _ = split_run(ctx, rows, 0.2, V.ZERO, frame_cuts(7), "seven inserts")
        seen.append(emits(cloud))
    same_emits(seen[0], seen[1])
    # the one-shot path finds no leftover state: on the same context, both sources
    want = V.downsample(rows, 0.2)
    same_emits({k: v for k, v in seen[0].items() if k != "sums"},
               {k: want[k] for k in ("keys", "counts", "rows", "f32")})
    check(ctx.voxel_downsample(as_batch(ctx, COUNTS, rows), 0.2), want, "one-shot, batch", n_points=len(rows))
    check(pkg().voxel_downsample(rows, 0.2, context=ctx), want, "one-shot, rows")
    small = f32(np.random.default_rng(8).uniform(-2, 2, (500, 4)))
    check(pkg().voxel_downsample(small, 0.5, context=ctx), V.downsample(small, 0.5), "one-shot, a smaller table in the larger blocks")
