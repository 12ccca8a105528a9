"""Shrinking a voxel cloud on the device: after any remove / subtract the cloud is bit for bit the restatement of
tests/voxelremove.py, which tests/test_voxel_remove_cpu.py holds to the one-shot restatement, and, where the definition
says so, a fresh voxel_downsample of what is left.  Every comparison is exact: keys, counts, the raw sums, the bits of
the float64 rows and of the float32 batch, and n_points.  A refused call names its item and leaves all of it as it was."""
import ctypes

import numpy as np
import pytest

import registration as R
import voxel as V
import voxelinsert as VI
import voxelremove as VR
from conftest import pkg

pytestmark = pytest.mark.gpu
H = 0.2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def emits(cloud):
    """Everything the cloud gives out, on the host."""
    b = cloud.batch()
    cols = np.stack(b.download_columns(), axis=1) if cloud.n_voxels else np.zeros((0, 4), np.float32)
    return dict(keys=cloud.keys(), counts=cloud.point_counts(), rows=cloud.rows(), f32=cols, sums=cloud.state().sums,
                n_points=np.array([cloud.n_points, cloud.n_voxels], np.int64))


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
    assert cloud.n_points == (int(want["counts"].sum()) if n_points is None else n_points), what
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


_cache = {}


def source(seed=1, n=6000, h=H, origin=V.ZERO):
    """6000 float32-exact points over 900 cells of the grid; nobody writes into it."""
    key = (seed, n, h, tuple(origin))
    if key not in _cache:
        rng = np.random.default_rng(seed)
        centre = rng.integers(-20, 20, (900, 3))
        pick = rng.integers(0, 900, n)
        rows = np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (n, 3))) * h, rng.uniform(-3, 3, n)])
        _cache[key] = f32(rows)
    return _cache[key]


def pair(ctx, rows, h=H, origin=V.ZERO):
    """The cloud of rows on the device and restated."""
    cloud, want = pkg().voxel_downsample(rows, h, origin, context=ctx), VR.Cloud(h, origin)
    want.insert(rows)
    return cloud, want


def voxel_of(rows, h=H, origin=V.ZERO):
    return V.pack(V.quantise(rows[:, :3], rows[:, 3], h, origin)[0])


def own_voxels(first, n, h=0.25, per=1):
    """n voxels of `per` points each, every one with its own key."""
    i = np.repeat(np.arange(first, first + n), per)
    keys = np.stack([i % 13 - 6, (i // 13) % 17 - 8, i // 221 - 4], axis=1)
    rng = np.random.default_rng(first + n)
    return f32(np.column_stack([(keys + rng.uniform(0.1, 0.9, (len(i), 3))) * h, rng.uniform(0, 1, len(i))]))


def remove_and_check(ctx, rows, mask_of, what, h=H, origin=V.ZERO):
    """remove(mask) against the restatement and against a fresh build of the rows that are left."""
    cloud, want = pair(ctx, rows, h, origin)
    mask = mask_of(cloud.n_voxels)
    gone = V.pack(want.keys[mask])
    assert cloud.remove(mask) == want.remove(mask) == int(mask.sum()), what
    got = check(cloud, want.result(), what)
    left = rows[~np.isin(voxel_of(rows, h, origin), gone)]
    assert cloud.n_points == len(left), what
    fresh = pkg().voxel_downsample(left, h, origin, context=ctx)
    same_emits(got, emits(fresh), (what, "fresh"))
    return len(left)


# ---- 1. remove ---------------------------------------------------------------------------------------------------------
def test_an_all_false_mask_changes_nothing(gpu_ctx):
    cloud, want = pair(gpu_ctx, source())
    before, slots = emits(cloud), table(gpu_ctx)
    assert cloud.remove(np.zeros(cloud.n_voxels, np.bool_)) == 0
    same_emits(emits(cloud), before)
    assert table(gpu_ctx) == slots
    check(cloud, want.result(), "all False", n_points=6000)


def test_an_all_true_mask_leaves_an_empty_cloud_that_insert_fills(gpu_ctx):
    ctx = gpu_ctx
    cloud, want = pair(ctx, source())
    M = cloud.n_voxels
    assert cloud.remove(np.ones(M, np.bool_)) == M == want.remove(np.ones(M, np.bool_))
    assert cloud.n_voxels == 0 and cloud.n_points == 0
    check(cloud, want.result(), "all True", n_points=0)
    assert cloud.state().keys.shape == (0, 3) and cloud.remove(np.zeros(0, np.bool_)) == 0
    assert table(ctx) == (1 << VR.table_shrink_log2(0, 14), 0)
    X = source(2)
    cloud.insert(as_batch(ctx, [2500, 0, 3500], X))
    got = check(cloud, V.downsample(X, H), "filled again", n_points=6000)
    same_emits(got, emits(pkg().voxel_downsample(X, H, context=ctx)), "fresh")


@pytest.mark.parametrize("what", ["alternate", "random tenth", "random nine tenths", "first", "last"])
def test_masks(gpu_ctx, what):
    rng = np.random.default_rng(12)
    masks = {"alternate": lambda M: np.arange(M) % 2 == 0, "random tenth": lambda M: rng.random(M) < 0.1,
             "random nine tenths": lambda M: rng.random(M) < 0.9, "first": lambda M: np.arange(M) == 0,
             "last": lambda M: np.arange(M) == M - 1}
    assert 0 < remove_and_check(gpu_ctx, source(), masks[what], what) < 6000


@pytest.mark.parametrize("M_keep", [255, 256, 257, 2047, 2048, 2049])
def test_survivor_counts_at_the_compaction_edges(gpu_ctx, M_keep):
    rows = own_voxels(0, M_keep + 3, per=2)

    def mask_of(M):
        assert M == M_keep + 3
        mask = np.zeros(M, np.bool_)
        mask[[0, M // 2, M - 1]] = True
        return mask
    assert remove_and_check(gpu_ctx, rows, mask_of, M_keep, h=0.25) == 2 * M_keep


def test_a_shrink_follows_the_rule_and_an_insert_grows_the_table_again(gpu_ctx):
    ctx, h = gpu_ctx, 0.25
    rows = own_voxels(0, 6000)
    cloud, want = pair(ctx, rows, h)
    assert table(ctx) == (16384, 0)
    # an eighth of 16 384 slots is 2048 survivors: the table stays at 2048 and shrinks at 2047
    for keep, log2 in ((2048, 14), (2047, 13), (100, 9)):
        mask = np.arange(cloud.n_voxels) >= keep
        log2cap = table(ctx)[0].bit_length() - 1
        assert cloud.remove(mask) == want.remove(mask)
        assert VR.table_shrink_log2(keep, log2cap) == log2 and table(ctx) == (1 << log2, 0), keep
        check(cloud, want.result(), ("kept", keep))
    more = own_voxels(6000, 1000)
    assert cloud.insert(more) == want.insert(more) == 1000
    assert table(ctx) == (1 << VI.table_log2(100, 1000, 9), 1) and VI.table_log2(100, 1000, 9) == 12
    check(cloud, want.result(), "grown again", n_points=1100)
    assert cloud.subtract(more) == want.subtract(more) == 1000
    assert table(ctx) == (1 << VR.table_shrink_log2(100, 12), 1) and VR.table_shrink_log2(100, 12) == 9
    check(cloud, V.downsample(rows[:100], h), "and shrunk", n_points=100)


# ---- 2. subtract -------------------------------------------------------------------------------------------------------
COUNTS = [900, 0, 1100, 1000]


def source_of(ctx, kind, rows, h=H, origin=V.ZERO):
    """rows (3000 of them) as a Batch of four frames, one of them empty, as they are, or as the VoxelSums of their cloud."""
    if kind == "batch":
        return as_batch(ctx, COUNTS, rows)
    if kind == "rows":
        return rows
    d = V.downsample(rows, h, origin)
    return pkg().VoxelSums(d["keys"], d["counts"], np.column_stack([d["S"], d["SI"]]), float(h), np.array(origin, np.float64))


def restated_subtract(want, kind, rows):
    if kind == "state":
        return want.subtract_records(*VI.records_of(V.downsample(rows, want.h, want.origin)))
    return want.subtract(rows)


@pytest.mark.parametrize("kind", ["batch", "rows", "state"])
def test_insert_then_subtract_is_the_identity(gpu_ctx, kind):
    ctx = gpu_ctx
    rows = source()
    base = rows[:3000]
    extra = np.concatenate([rows[3000:4500], source(3)[:1500]])      # voxels it shares with base, and 1500 points of its own cells
    cloud, want = pair(ctx, base)
    before = emits(cloud)
    src = source_of(ctx, kind, extra)
    grown = cloud.merge(src) if kind == "state" else cloud.insert(src)
    assert grown > 0 and cloud.n_points == 6000
    cloud.normals(2 * H)
    assert cloud.subtract(src) == grown
    same_emits(emits(cloud), before, kind)
    check(cloud, want.result(), kind, n_points=3000)


@pytest.mark.parametrize("kind", ["batch", "rows", "state"])
def test_the_remainder_of_a_cloud_minus_its_head(gpu_ctx, kind):
    ctx = gpu_ctx
    rows = source()
    A, B = rows[:3000], rows[3000:]
    cloud, want = pair(ctx, rows)
    emptied = restated_subtract(want, kind, A)
    assert cloud.subtract(source_of(ctx, kind, A)) == emptied > 0
    got = check(cloud, want.result(), kind, n_points=3000)
    # the records of a build of B, which may number them differently
    fresh = V.downsample(B, H)
    a, b = np.argsort(V.pack(got["keys"])), np.argsort(V.pack(fresh["keys"]))
    assert np.array_equal(got["keys"][a], fresh["keys"][b]) and np.array_equal(got["counts"][a], fresh["counts"][b])
    assert np.array_equal(got["sums"][a], np.column_stack([fresh["S"], fresh["SI"]])[b])
    assert np.array_equal(bits(got["rows"][a]), bits(fresh["rows"][b])) and not np.array_equal(a, b)


def test_a_call_that_empties_no_voxel_touches_no_id_and_no_table(gpu_ctx):
    ctx = gpu_ctx
    rows = source()
    cloud, want = pair(ctx, rows)
    vox = voxel_of(rows)
    _, first = np.unique(vox, return_index=True)
    rest = np.ones(len(rows), np.bool_)
    rest[first] = False                                  # every voxel keeps its first point
    part = rows[rest][:2900]
    keys, slots = cloud.keys(), table(ctx)
    ctx.read_timing_voxel_remove()
    ctx.timing(True)
    try:
        assert cloud.subtract(as_batch(ctx, [1000, 0, 1900], part)) == 0 == want.subtract(part)
    finally:
        ctx.timing(False)
    t = ctx.read_timing_voxel_remove()
    assert t["regions"] == 3 and t["compact_ms"] == 0.0 and all(0.0 < t[k] < 1000.0 for k in ("validate_ms", "apply_ms", "check_ms")), t
    assert np.array_equal(cloud.keys(), keys) and table(ctx) == slots
    check(cloud, want.result(), "no voxel emptied", n_points=len(rows) - 2900)
    # and one that empties some runs the compaction: everything that is left of fifty voxels
    still = np.ones(len(rows), np.bool_)
    still[np.flatnonzero(rest)[:2900]] = False
    last = rows[still & np.isin(vox, vox[first][:50])]
    ctx.timing(True)
    try:
        gone = cloud.subtract(last)
    finally:
        ctx.timing(False)
    t = ctx.read_timing_voxel_remove()
    assert gone == want.subtract(last) == 50 and t["regions"] == 6 and t["compact_ms"] > 0.0, t
    check(cloud, want.result(), "some emptied")
    assert ctx.read_timing_voxel_remove()["regions"] == 0


def test_the_same_key_many_times_in_one_call(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(4)
    one = f32(np.column_stack([rng.uniform(0.21, 0.39, (3000, 3)), rng.uniform(0, 1, 3000)]))      # voxel (1, 1, 1)
    rows = np.concatenate([source()[:500], one, one[:7]])
    cloud, want = pair(ctx, rows)
    assert cloud.subtract(one) == want.subtract(one) == 0
    got = check(cloud, want.result(), "3000 items of one voxel", n_points=507)
    assert 7 in got["counts"].tolist()
    assert cloud.subtract(as_batch(ctx, [7], one[:7])) == want.subtract(one[:7]) == 1
    check(cloud, V.downsample(rows[:500], H), "and its last seven", n_points=500)


# ---- 3. every refusal names its item and changes nothing ----------------------------------------------------------------
def refused(cloud, before, src, restated, index, reason, match):
    with pytest.raises(V.Refused) as e:
        restated()
    assert (e.value.index, e.value.reason) == (index, reason), match
    with pytest.raises(ValueError, match=match):
        cloud.subtract(src)
    same_emits(emits(cloud), before, match)
    return e.value


def test_every_refusal(gpu_ctx):
    m, ctx = pkg(), gpu_ctx
    rows = source()
    held = rows[:3000]
    cloud, want = pair(ctx, held)
    before, slots = emits(cloud), table(ctx)
    at = 900 + 5                                          # frame 2, point 5
    for kind in ("batch", "rows"):
        name = "frame 2, point 5 " if kind == "batch" else f"row {at} "
        # a NaN row, the lowest of several
        bad = held.copy()
        bad[[at, at + 300], 1] = np.nan
        refused(cloud, before, source_of(ctx, kind, bad), lambda: want.subtract(bad), at, VR.ITEM, name + r".*not finite")
        # a point of a voxel the cloud lacks, the lowest of several, and below a later NaN
        away = held.copy()
        away[[at, at + 1, 2999], 0] += 100.0
        away[at + 50, 2] = np.nan
        refused(cloud, before, source_of(ctx, kind, away), lambda: want.subtract(away), at, VR.MISSING, name + r".*holds no voxel")
    # more points than the cloud holds
    refused(cloud, before, np.concatenate([held, held[:1]]), lambda: want.subtract(np.concatenate([held, held[:1]])), -1,
            VR.POINTS, r"brings 3001 points and the cloud holds 3000")
    # one more point of a voxel than it holds
    vox = voxel_of(held)
    mine, other = held[vox == vox[5]], held[vox != vox[5]][:3]
    over = np.concatenate([other, mine, mine[:1]])
    e = refused(cloud, before, over, lambda: want.subtract(over), 3, VR.REMAINDER, r"row 3 .*no set of points")
    with pytest.raises(ValueError, match=r"voxel \(%d, %d, %d\)" % e.key):
        cloud.subtract(over)
    # a state of another grid, a bad record, a record the cloud lacks, and a count of 0 left with a sum
    state = source_of(ctx, "state", held)
    rec = VI.records_of(V.downsample(held, H))
    with pytest.raises(ValueError, match="bit for bit"):
        cloud.subtract(state._replace(voxel=float(np.nextafter(H, 1.0))))
    counts = state.counts.copy()
    counts[17] = 0
    refused(cloud, before, state._replace(counts=counts),
            lambda: want.subtract_records(rec[0], counts.astype(np.int64), rec[2], rec[3]), 17, VR.ITEM, r"record 17 .*a count below 1")
    keys = state.keys.copy()
    keys[23] += 4000
    refused(cloud, before, state._replace(keys=keys), lambda: want.subtract_records(keys, *rec[1:]), 23, VR.MISSING,
            r"record 23 .*holds no voxel")
    sums = state.sums.copy()
    sums[9, 3] -= 1
    refused(cloud, before, state._replace(sums=sums), lambda: want.subtract_records(rec[0], rec[1], sums[:, :3], sums[:, 3]), 9,
            VR.REMAINDER, r"record 9 .*no set of points")
    # a mask of the wrong shape or dtype
    for mask in (np.zeros(cloud.n_voxels + 1, np.bool_), np.zeros(cloud.n_voxels, np.uint8), np.zeros((cloud.n_voxels, 1), np.bool_)):
        with pytest.raises(ValueError, match="bool array of shape"):
            cloud.remove(mask)
    same_emits(emits(cloud), before, "masks")
    assert table(ctx) == slots and cloud.n_points == 3000
    # the library's own out words
    buf = ctx.device_buffer(32)
    buf.from_host(np.array([[500.0, 0.0, 0.0, 0.0]]))
    gone, row, why = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int32(7)
    rc = ctx.lib.mc_voxel_subtract_f64(ctx.handle, buf.ptr, 4, 1, ctypes.byref(gone), ctypes.byref(row), ctypes.byref(why))
    assert (rc, gone.value, row.value, why.value) == (m._lib.MC_ERR_INVALID, 0, 0, VR.WHY[VR.MISSING])
    assert ctx.lib.mc_voxel_subtract_f64(ctx.handle, None, 4, 0, ctypes.byref(gone), ctypes.byref(row), ctypes.byref(why)) == 0
    assert (gone.value, row.value, why.value) == (0, -1, 0)
    bare = m.Context(0)
    assert bare.lib.mc_voxel_remove(bare.handle, None, ctypes.byref(gone)) == m._lib.MC_ERR_STATE
    assert bare.lib.mc_voxel_subtract_f64(bare.handle, None, 4, 0, ctypes.byref(gone), ctypes.byref(row), None) == m._lib.MC_ERR_STATE
    # the cloud still works: the whole of it leaves, and a cloud without voxels holds none
    assert cloud.subtract(state) == want.subtract_records(*rec) == len(rec[0]) and cloud.n_voxels == 0 and cloud.n_points == 0
    with pytest.raises(ValueError, match=r"row 0 .*holds no voxel"):
        cloud.subtract(held[:2])
    empty = m.voxel_downsample(np.zeros((0, 4)), H, context=ctx)
    with pytest.raises(ValueError, match=r"row 0 .*holds no voxel"):
        empty.subtract(held[:2])
    assert empty.subtract(np.zeros((0, 4))) == 0 and empty.remove(np.zeros(0, np.bool_)) == 0
    # a closed cloud
    empty.close()
    for call in (lambda: empty.remove(np.zeros(0, np.bool_)), lambda: empty.subtract(held[:2]), lambda: empty.subtract(state)):
        with pytest.raises(ValueError, match="closed or was replaced"):
            call()


def test_counts_that_fit_but_a_sum_that_cannot(gpu_ctx):
    """A voxel of two points at its low corner, minus one point near its high corner: a count of 1, a sum below 0."""
    ctx = gpu_ctx
    rows = f32(np.array([[0.01, 0.01, 0.01, 0.0], [0.02, 0.02, 0.02, 0.0], [5.1, 5.1, 5.1, 1.0]]))
    cloud, want = pair(ctx, rows)
    before = emits(cloud)
    take = f32(np.array([[5.1, 5.1, 5.1, 1.0], [0.19, 0.19, 0.19, 0.0]]))
    for src, name in ((take, "row 1 "), (as_batch(ctx, [1, 1], take), "frame 1, point 0 ")):
        e = refused(cloud, before, src, lambda: want.subtract(take), 1, VR.REMAINDER, name + r".*voxel \(0, 0, 0\)")
        assert e.key == (0, 0, 0)
    assert cloud.n_points == 3 and cloud.n_voxels == 2
    assert cloud.subtract(rows[2:]) == want.subtract(rows[2:]) == 1
    check(cloud, V.downsample(rows[:2], H), "the other voxel left", n_points=2)


# ---- 4. the analyses see the shrunk cloud ------------------------------------------------------------------------------
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


def test_the_analyses_see_the_shrunk_cloud(gpu_ctx):
    m, ctx, h = pkg(), gpu_ctx, R.H
    rows = R.corner_rows()
    src = R.moved_back(R.corner_source(1000, 3), R.NEARBY)
    # the cloud without its first plane, against a fresh build of the rows of the other voxels
    cloud = m.voxel_downsample(rows, h, context=ctx)
    M = cloud.n_voxels
    cloud.clusters(2 * h, 3)
    plane = cloud.segment_plane(h, 200)
    gone = V.pack(cloud.keys()[plane.inliers])
    assert 200 <= plane.n_inliers < M and cloud.remove(plane.inliers) == plane.n_inliers and cloud.n_voxels == M - plane.n_inliers
    got_cloud, got = emits(cloud), analyses(cloud, src, h)
    left = rows[~np.isin(voxel_of(rows, h), gone)]
    fresh = m.voxel_downsample(left, h, context=ctx)
    same_emits(got_cloud, emits(fresh))
    want = analyses(fresh, src, h)
    same_results(got, want)
    assert want["plane"].n_inliers >= 200 and want["register"].pairs > 100 and len(want["normals"].normals) == M - plane.n_inliers
    # insert(B); subtract(B): the ids coincide with the cloud's before, analysed in between
    extra = np.column_stack([R.corner_source(700, 5) + 0.3, np.full(700, 0.25)])
    assert fresh.insert(extra) > 0
    assert len(fresh.normals(2 * h).normals) == fresh.n_voxels and fresh.clusters(2 * h, 3).n_clusters >= 1
    assert fresh.subtract(extra) > 0
    same_emits(emits(fresh), got_cloud)
    same_results(analyses(fresh, src, h), want)


# ---- 5. off the default origin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2])
def test_off_the_default_origin(gpu_ctx, grid):
    ctx = gpu_ctx
    h, origin = V.GRIDS[grid]
    rng = np.random.default_rng(grid)
    centre = rng.integers(-20, 20, (900, 3))
    pick = rng.integers(0, 900, 6000)
    rows = np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (6000, 3))) * h + np.array(origin), rng.uniform(-3, 3, 6000)])
    assert 0 < remove_and_check(ctx, rows, lambda M: np.arange(M) % 3 == 0, "remove", h, origin) < 6000
    cloud, want = pair(ctx, rows, h, origin)
    assert cloud.subtract(rows[:3000]) == want.subtract(rows[:3000]) > 0
    got = check(cloud, want.result(), "subtract", n_points=3000)
    fresh = V.downsample(rows[3000:], h, origin)
    a, b = np.argsort(V.pack(got["keys"])), np.argsort(V.pack(fresh["keys"]))
    assert np.array_equal(got["sums"][a], np.column_stack([fresh["S"], fresh["SI"]])[b])
    assert np.array_equal(bits(got["rows"][a]), bits(fresh["rows"][b]))
    before = emits(cloud)
    cloud.insert(rows[:700])
    cloud.subtract(rows[:700])
    same_emits(emits(cloud), before, "identity")
