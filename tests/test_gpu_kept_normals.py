"""The normals a voxel cloud keeps across its edits, on the device (include/mcdeskew.h "kept normals"): after every
edit ``kept_normals()`` is a fresh ``normals(radius, max_nn)`` in the bits of the normals, the curvature and the counts,
and ``kept.refreshed_last`` is the size of the dirty set D of the restatement (tests/keptnormals.py, held to the
definition by tests/test_kept_normals_cpu.py).  Unless a case says otherwise its inputs make |D| < M / 2, which the
check asserts: a case in which everything is dirty shows nothing about carrying rows over."""
import ctypes

import numpy as np
import pytest

import keptnormals as K
import normals as N
import registration as G
import voxel as V
from conftest import pkg

pytestmark = pytest.mark.gpu
H = 0.25


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def raw(n):
    """The bytes of a VoxelNormals."""
    return n.normals.tobytes() + n.curvature.tobytes() + n.counts.tobytes()


def table(ctx):
    slots, growths = ctypes.c_int64(-1), ctypes.c_int64(-1)
    pkg()._lib.check(ctx.lib.mc_voxel_table(ctx.handle, ctypes.byref(slots), ctypes.byref(growths)), "table")
    return slots.value, growths.value


def state_of(m, recs, h, origin=V.ZERO):
    keys, n, S, SI = recs
    return m.VoxelSums(np.ascontiguousarray(keys, np.int32), np.ascontiguousarray(n, np.int32),
                       np.ascontiguousarray(np.column_stack([S, SI]), np.int64), float(h), np.array(origin, np.float64))


class Kept:
    """A cloud on the device that keeps its normals, and its restatement."""

    def __init__(self, ctx, rows, rel=2.0, max_nn=30, h=H):
        self.m, self.ctx, self.h, self.radius, self.max_nn, self.R = pkg(), ctx, h, rel * h, max_nn, int(np.ceil(rel))
        self.cloud = self.m.voxel_downsample(rows, h, context=ctx)
        self.want = K.Cloud.of_rows(rows, h)
        self.cloud.keep_normals(self.radius, max_nn)
        k = self.cloud.kept
        assert (k.radius, k.max_nn, k.full_passes, k.refreshed_last, k.refreshed_total) == (self.radius, max_nn, 1, 0, 0)
        self.total = 0
        self.fresh("kept")

    def fresh(self, what):
        """kept_normals() against a fresh normals(): -> the kept ones."""
        kept, fresh = self.cloud.kept_normals(), self.cloud.normals(self.radius, self.max_nn)
        assert kept.covariance is None and len(kept.counts) == self.cloud.n_voxels == len(self.want), what
        assert np.array_equal(bits(kept.normals), bits(fresh.normals)), what
        assert np.array_equal(bits(kept.curvature), bits(fresh.curvature)), what
        assert np.array_equal(kept.counts, fresh.counts), what
        return kept

    def done(self, edit, what, half=True):
        """After the device's edit: the restatement's, D, and the checks of the module docstring."""
        D = K.dirty(edit, self.R)
        self.want = edit.after
        assert np.array_equal(self.cloud.keys(), edit.after.keys), what
        k = self.cloud.kept
        assert k.refreshed_last == len(D), (what, k.refreshed_last, len(D))
        self.total += len(D)
        assert k.refreshed_total == self.total and k.full_passes == 1, what
        if half:
            assert len(D) < len(edit.after) / 2, (what, len(D), len(edit.after))
        self.fresh(what)
        return D

    def insert(self, rows, what, half=True, src=None):
        self.cloud.insert(rows if src is None else src)
        return self.done(K.add(self.want, K.items_of_rows(self.want, rows)), what, half)

    def merge(self, recs, what, half=True):
        self.cloud.merge(state_of(self.m, recs, self.h))
        return self.done(K.add(self.want, recs), what, half)

    def subtract(self, rows, what, half=True):
        self.cloud.subtract(rows)
        return self.done(K.subtract(self.want, K.items_of_rows(self.want, rows)), what, half)

    def subtract_records(self, recs, what, half=True):
        self.cloud.subtract(state_of(self.m, recs, self.h))
        return self.done(K.subtract(self.want, recs), what, half)

    def remove(self, mask, what, half=True):
        assert self.cloud.remove(mask) == int(mask.sum())
        return self.done(K.remove(self.want, mask), what, half)


def far(n=12):
    """n voxels nothing else is near to: what makes a small case's cloud more than twice its dirty set."""
    return K.cells_rows(np.stack([200 + 12 * np.arange(n), np.full(n, -90), np.full(n, 33)], axis=1), H)


# ---- the window's edge -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 4])
def test_window_edge(gpu_ctx, R):
    """A point inserted into a new voxel exactly R cells from a voxel, on each axis and in both directions, makes that
    voxel dirty; R + 1 cells away it does not."""
    k = Kept(gpu_ctx, np.concatenate([K.cells_rows([[0, 0, 0]], H), far()]), rel=float(R))
    for axis in range(3):
        for sign in (1, -1):
            for d, size in ((R, 2), (R + 1, 1)):
                cell = np.zeros((1, 3), np.int64)
                cell[0, axis] = sign * d
                row = K.cells_rows(cell, H)
                D = k.insert(row, (R, axis, sign, d))
                assert D.tolist() == ([0, len(k.want) - 1] if size == 2 else [len(k.want) - 1])
                D = k.subtract(row, (R, axis, sign, d, "back"))
                assert D.tolist() == ([0] if size == 2 else [])


@pytest.mark.parametrize("R", [1, 2, 4])
def test_key_range(gpu_ctx, R):
    """The same at both ends of the key range: N.key_ends()'s voxels at kx = -2^20 and ky = 2^20 - 1, with decoys where a
    key packed without the range check would land; an item into each voxel in turn, then new voxels R and R + 1 cells
    along the range's end."""
    rows, h = N.key_ends()[:2]
    k = Kept(gpu_ctx, np.concatenate([rows, K.cells_rows([[300, 300, 300], [-300, 300, 300], [300, -300, 300]], h)]), rel=float(R), h=h)
    for v in range(8):
        k.insert(rows[v:v + 1], (R, v))
    assert k.insert(rows[3:4], (R, "ky end")).tolist() == [3, 4, 5]           # not the decoys 6 and 7
    for end, along in (([V.KEY_MIN, 5, 5], 1), ([10, V.KEY_END - 1, -3], 2)):
        for d in (R, R + 1):
            for sign in (1, -1):
                cell = np.array([end])
                cell[0, along] += sign * (d + 1)        # beside the end's own neighbours: a new voxel
                row = K.cells_rows(cell, h)
                k.insert(row, (R, end, d, sign))
                k.subtract(row, (R, end, d, sign, "back"))


# ---- what a refresh must see ---------------------------------------------------------------------------------------------
def test_count_two_to_three_and_back(gpu_ctx):
    """A new voxel raises a neighbour's count from 2 to 3, so its normal leaves (0, 0, 1); the subtraction that empties the
    new voxel takes it back."""
    k = Kept(gpu_ctx, np.concatenate([K.cells_rows([[0, 0, 0], [1, 0, 0]], H), far()]))
    before = k.cloud.kept_normals()
    assert before.counts[:2].tolist() == [2, 2] and before.normals[0].tolist() == [0.0, 0.0, 1.0]
    new = K.cells_rows([[0, 0, 1]], H)
    assert k.insert(new, "third").tolist() == [0, 1, len(k.want) - 1]
    after = k.cloud.kept_normals()
    assert after.counts[[0, 1, -1]].tolist() == [3, 3, 3] and after.normals[0].tolist() == [0.0, 1.0, 0.0]
    assert k.subtract(new, "and back").tolist() == [0, 1]
    assert raw(k.cloud.kept_normals()) == raw(before)


def test_radius_flip_without_a_new_voxel(gpu_ctx):
    """An insert into an existing voxel moves its centroid across another voxel's d2 <= r2 decision."""
    rows = np.concatenate([K.cells_rows([[0, 0, 0], [1, 0, 0]], H), far()])
    rows[1, 0] += 0.02 * H                                       # 1.02 h from voxel 0: outside the radius of h
    k = Kept(gpu_ctx, rows, rel=1.0)
    assert k.cloud.kept_normals().counts[:2].tolist() == [1, 1]
    more = rows[1:2].copy()
    more[0, 0] -= 0.08 * H                                       # the centroid moves to 0.98 h
    assert k.cloud.n_voxels == len(rows)
    assert k.insert(more, "flip").tolist() == [0, 1] and k.cloud.n_voxels == len(rows)
    assert k.cloud.kept_normals().counts[:2].tolist() == [2, 2]
    assert k.subtract(more, "flop").tolist() == [0, 1] and k.cloud.kept_normals().counts[:2].tolist() == [1, 1]


def cap_case(max_nn):
    """-> the rows of a cloud in which voxel X has exactly max_nn neighbours, X's id, and two rows that each add one."""
    if max_nn == 30:
        rows, h, radius = N.block()                              # h = 0.5, radius = 2 h: 33 neighbours inside
        cells = np.floor(rows[:, :3] / h).astype(np.int64)
        out = np.array([[5, 3, 3], [3, 5, 3], [3, 3, 5]])        # three of X's six neighbours at two cells
        gone = (cells[:, None, :] == out[None]).all(axis=2).any(axis=1)
        return rows[~gone], h, 2.0, [3, 3, 3], K.cells_rows(out[:1], h), K.cells_rows(out[1:2], h)
    cells = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0]])
    return (np.concatenate([K.cells_rows(cells, H), far()]), H, 1.0, [0, 0, 0], K.cells_rows([[0, 1, 0]], H),
            K.cells_rows([[0, -1, 0]], H))


@pytest.mark.parametrize("max_nn", [3, 30])
def test_the_cap_through_the_list(gpu_ctx, max_nn):
    """One insert pushes a voxel from max_nn to max_nn + 1 neighbours, a second refreshes it when it is capped already:
    the cap kernel on the dirty list's voxels."""
    rows, h, rel, x_cell, first, second = cap_case(max_nn)
    k = Kept(gpu_ctx, rows, rel=rel, max_nn=max_nn, h=h)
    x = int(np.flatnonzero((k.want.keys == x_cell).all(axis=1))[0])
    found = lambda: int(k.want.estimate(k.radius, 0)["counts"][x])      # without the cap
    assert found() == max_nn and k.cloud.kept_normals().counts[x] == max_nn
    assert x in k.insert(first, "over the cap") and found() == max_nn + 1
    assert x in k.insert(second, "capped already") and found() == max_nn + 2
    assert k.cloud.kept_normals().counts[x] == max_nn
    k.subtract(np.concatenate([first, second]), "and back")
    assert found() == max_nn


def units():
    """180 corners of three voxels (mutual neighbours at radius 2 h, each with its own normal) and 4 single voxels, nine
    cells apart: -> rows, the row of the first voxel of every corner, the rows of the singles."""
    i = np.arange(180)
    base = np.stack([9 * (i % 14), 9 * (i // 14), np.zeros(180, np.int64)], axis=1)
    cells = (base[:, None, :] + np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]])[None]).reshape(-1, 3)
    singles = np.stack([9 * np.arange(4), np.full(4, -30), np.zeros(4, np.int64)], axis=1)
    rng = np.random.default_rng(180)
    return K.cells_rows(np.concatenate([cells, singles]), H, rng), 3 * i, 540 + np.arange(4)


@pytest.mark.parametrize("n_dirty", [1, 63, 64, 65, 255, 256, 257])
def test_dirty_counts_at_the_launch_edges(gpu_ctx, n_dirty):
    rows, corners, singles = units()
    k = Kept(gpu_ctx, rows)
    rng = np.random.default_rng(n_dirty)
    at = np.concatenate([corners[:n_dirty // 3], singles[:n_dirty % 3]])
    frame = rows[at].copy()
    frame[:, :3] += rng.uniform(-0.1, 0.1, (len(at), 3)) * H
    assert len(k.insert(frame, n_dirty)) == n_dirty
    assert len(k.subtract(frame, (n_dirty, "back"))) == n_dirty


def test_an_insert_that_grows_the_table(gpu_ctx):
    rows = K.sheet(200, seed=3, h=H)
    k = Kept(gpu_ctx, rows)
    assert table(gpu_ctx) == (512, 0)
    rng = np.random.default_rng(4)
    frame = np.repeat(rows[[5, 50, 100, 150, 199]], 20, axis=0)
    frame[:, :3] += rng.uniform(-0.1, 0.1, (100, 3)) * H
    k.insert(frame, "grown")
    assert table(gpu_ctx) == (1024, 1) and k.cloud.n_voxels == 200
    k.insert(K.cells_rows([[60, 60, 60], [0, 0, 1]], H), "new voxels in the grown table")


def test_three_hundred_inserts_in_a_row(gpu_ctx):
    rows = K.sheet(600, seed=9, h=H)
    k = Kept(gpu_ctx, rows)
    rng = np.random.default_rng(10)
    lo, hi = k.want.keys.min(axis=0), k.want.keys.max(axis=0) + 1
    for i in range(300):
        cell = k.want.keys[[rng.integers(0, len(k.want))]] if i % 2 else rng.integers(lo, hi, (1, 3))
        k.insert(K.cells_rows(cell, H, rng), i)
    assert k.cloud.kept.refreshed_total == k.total > 300 and len(k.want) > 600


# ---- removals ------------------------------------------------------------------------------------------------------------
def halves(M=1200, seed=11):
    """A sheet one cell thick whose even ids lie in x < 0 and whose odd ids in x >= 0: -> rows"""
    rows = K.sheet(M, seed, H, thick=1)
    left, right = rows[rows[:, 0] < 0], rows[rows[:, 0] >= 0]
    n = min(len(left), len(right))
    out = np.empty((2 * n, 4))
    out[0::2], out[1::2] = left[:n], right[:n]
    return out


@pytest.mark.parametrize("what", ["alternate", "random tenth", "first", "last"])
def test_masks(gpu_ctx, what):
    """Carried rows sit at their new ids: every survivor's id changes under all but the last mask."""
    rng = np.random.default_rng(12)
    masks = {"alternate": lambda M: np.arange(M) % 2 == 0, "random tenth": lambda M: rng.random(M) < 0.1,
             "first": lambda M: np.arange(M) == 0, "last": lambda M: np.arange(M) == M - 1}
    k = Kept(gpu_ctx, halves(), rel=1.0)
    D = k.remove(masks[what](len(k.want)), what)
    assert len(D) > 0


@pytest.mark.parametrize("M_keep", [255, 256, 257])
def test_survivor_counts_at_the_compaction_edges(gpu_ctx, M_keep):
    k = Kept(gpu_ctx, K.sheet(M_keep + 3, seed=M_keep, h=H, thick=1), rel=1.0)
    mask = np.zeros(M_keep + 3, np.bool_)
    mask[[0, (M_keep + 3) // 2, M_keep + 2]] = True
    k.remove(mask, M_keep)
    assert k.cloud.n_voxels == M_keep


def test_a_removal_that_shrinks_the_table(gpu_ctx):
    k = Kept(gpu_ctx, K.sheet(2100, seed=21, h=H, thick=1), rel=1.0)
    assert table(gpu_ctx) == (8192, 0)
    x = k.want.keys[:, 0]
    mask = x > np.sort(x)[799]                                   # the 800 voxels of lowest x stay, at least
    k.remove(mask, "shrunk")
    assert table(gpu_ctx) == (4096, 0) and 800 <= k.cloud.n_voxels < 1024      # >= 4 M'
    k.insert(K.sheet(2100, seed=21, h=H, thick=1)[:40], "and an insert afterwards")


def test_an_emptied_cloud_filled_again(gpu_ctx):
    """An all-True mask, then an insert into the empty cloud: every voxel is new, so |D| = M (exempt from the half rule)."""
    rows = K.sheet(300, seed=30, h=H)
    k = Kept(gpu_ctx, rows)
    assert k.remove(np.ones(300, np.bool_), "all True", half=False).tolist() == []
    assert k.cloud.n_voxels == 0 and k.cloud.kept is not None and len(k.cloud.kept_normals().counts) == 0
    assert k.remove(np.zeros(0, np.bool_), "nothing of nothing", half=False).tolist() == []
    D = k.insert(K.sheet(300, seed=31, h=H), "filled again", half=False)
    assert len(D) == 300 == k.cloud.n_voxels
    k.cloud.drop_normals()
    empty = pkg().voxel_downsample(np.zeros((0, 4)), H, context=gpu_ctx)      # the way to start a map from nothing
    empty.keep_normals()
    assert empty.kept.radius == 2 * H and empty.insert(rows) == 300 and empty.kept.refreshed_last == 300
    assert raw(empty.kept_normals()) == raw(empty.normals(2 * H, 30))


def test_an_all_false_mask_recomputes_nothing(gpu_ctx):
    k = Kept(gpu_ctx, K.sheet(300, seed=32, h=H))
    k.insert(K.cells_rows(k.want.keys[[7]], H), "something first")
    before = k.cloud.kept_normals()
    assert k.cloud.remove(np.zeros(300, np.bool_)) == 0
    assert k.cloud.kept.refreshed_last == 0 and raw(k.cloud.kept_normals()) == raw(before)


# ---- identities and refusals -------------------------------------------------------------------------------------------------
def frame_for(want, rng, new=6, old=30):
    lo, hi = want.keys.min(axis=0), want.keys.max(axis=0) + 1
    return f32(np.concatenate([K.cells_rows(rng.integers(lo, hi, (new, 3)), H, rng),
                               K.cells_rows(want.keys[rng.integers(0, len(want), old)], H, rng)]))


def test_insert_then_subtract_and_merge_then_subtract_are_the_identity(gpu_ctx):
    k = Kept(gpu_ctx, K.sheet(1500, seed=40, h=H))
    rng = np.random.default_rng(41)
    before = k.cloud.kept_normals()
    B = frame_for(k.want, rng)
    batch = gpu_ctx.batch([20, 0, 16])
    batch.upload_columns(*[B[:, c].astype(np.float32) for c in range(4)])
    k.insert(B, "insert a batch", src=batch)
    assert k.cloud.n_voxels > 1500                               # the subtraction empties the new voxels
    k.subtract(B, "subtract it")
    assert raw(k.cloud.kept_normals()) == raw(before) and k.cloud.n_voxels == 1500
    other = K.Cloud.of_rows(frame_for(k.want, rng), H)
    recs = other.records(np.arange(len(other)))
    k.merge(recs, "merge")
    assert k.cloud.n_voxels > 1500
    k.subtract_records(recs, "unmerge")
    assert raw(k.cloud.kept_normals()) == raw(before) and k.cloud.n_voxels == 1500


def test_every_refusal_leaves_the_kept_rows(gpu_ctx):
    m = pkg()
    k = Kept(gpu_ctx, K.sheet(400, seed=50, h=H))
    rng = np.random.default_rng(51)
    good = frame_for(k.want, rng)
    here = K.cells_rows(k.want.keys[[3]], H)
    nowhere = K.cells_rows([[500, 500, 500]], H)
    nan = good.copy()
    nan[17, 1] = np.nan
    recs = k.want.records([3, 4])
    count0 = (recs[0], np.array([1, 0]), recs[2], recs[3])
    too_many = (recs[0][:1], np.array([2 ** 31 - 1 - 400]), np.zeros((1, 3), np.int64), np.zeros(1, np.int64))
    twice = (recs[0], 2 * recs[1], 2 * recs[2], 2 * recs[3])
    refused = [("insert: a bad point", lambda: k.cloud.insert(nan)),
               ("merge: a bad record", lambda: k.cloud.merge(state_of(m, count0, H))),
               ("merge: 2^31 points", lambda: k.cloud.merge(state_of(m, too_many, H))),
               ("subtract: a bad point", lambda: k.cloud.subtract(nan)),
               ("subtract: a missing voxel", lambda: k.cloud.subtract(np.concatenate([good[-5:], nowhere]))),
               ("subtract: a bad remainder", lambda: k.cloud.subtract(np.concatenate([here, here]))),
               ("subtract: a bad remainder of records", lambda: k.cloud.subtract(state_of(m, twice, H))),
               ("subtract: a bad record", lambda: k.cloud.subtract(state_of(m, count0, H)))]
    for what, call in refused:
        assert len(k.insert(here, "an edit that refreshes")) > 0 and k.cloud.kept.refreshed_last > 0
        before, total = k.cloud.kept_normals(), k.cloud.kept.refreshed_total
        with pytest.raises(ValueError):
            call()
        after = k.cloud.kept
        assert (after.refreshed_last, after.refreshed_total, after.full_passes) == (0, total, 1), what
        assert raw(k.cloud.kept_normals()) == raw(before), what
        k.fresh(what)
        k.subtract(here, "and the edit back")                    # voxel 3 holds two points whenever a call is refused
    whole = k.want.records(np.arange(len(k.want)))
    with pytest.raises(ValueError, match="more points than it holds"):
        k.cloud.subtract(state_of(m, (whole[0], whole[1] + 1, whole[2], whole[3]), H))
    assert k.cloud.kept.refreshed_last == 0
    k.fresh("more points than the cloud holds")


# ---- registration ----------------------------------------------------------------------------------------------------------
def reg_raw(r):
    return b"".join(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode() for v in r)


def registrations(cloud, src, batch, **kw):
    return reg_raw(cloud.register(src, 2 * H, max_iterations=4, **kw)) + reg_raw(cloud.register_frames(batch, 2 * H, max_iterations=4, **kw))


def test_registration_reads_the_kept_normals(gpu_ctx):
    """register and register_frames on a cloud that keeps the call's normals against the same calls on a second context
    that keeps none: equal in every field, the history included, across edits and after drop_normals; one full pass."""
    m = pkg()
    other = m.Context(0)
    rows = G.corner_rows()
    src = f32(G.moved_back(G.corner_source(900, 900), G.KNOWN))
    clouds = [m.voxel_downsample(rows, H, context=ctx) for ctx in (gpu_ctx, other)]
    batches = []
    for ctx in (gpu_ctx, other):
        b = ctx.batch([400, 0, 500])
        b.upload_columns(*[src[:, c].astype(np.float32) for c in range(3)], np.zeros(900, np.float32))
        batches.append(b)
    kept, plain = clouds
    kept.keep_normals()                                          # 2 h and 30: register's defaults
    assert plain.kept is None and kept.kept.radius == 2 * H
    gpu_ctx.timing(True)
    gpu_ctx.read_timing_register(), gpu_ctx.read_timing_register_frames(), gpu_ctx.read_timing_normals()

    def agree(what, **kw):
        a, b = (registrations(c, src, batch, **kw) for c, batch in zip(clouds, batches))
        assert a == b, what
        return a
    try:
        first = agree("as built")
        t = gpu_ctx.read_timing_register(), gpu_ctx.read_timing_register_frames(), gpu_ctx.read_timing_normals()
        assert t[0]["normals_ms"] == 0.0 and t[1]["normals_ms"] == 0.0 and t[2]["window_ms"] == 0.0      # no normals kernel ran
        assert t[0]["correspond_ms"] > 0.0
    finally:
        gpu_ctx.timing(False)
    moved = f32(np.column_stack([G.move(G.KNOWN, src[:300]), np.full(300, 0.5)]))
    mask = np.arange(kept.n_voxels) % 7 == 0
    for c in clouds:
        c.insert(moved)
    assert 0 < kept.kept.refreshed_last and agree("after an insert") != first
    for c in clouds:
        c.subtract(moved[:100])
    agree("after a subtraction")
    for c in clouds:
        assert c.remove(mask) == int(mask.sum())
    agree("after a removal")
    assert kept.kept.full_passes == 1 and raw(kept.kept_normals()) == raw(plain.normals(2 * H, 30))
    kept.drop_normals()
    assert kept.kept is None
    with pytest.raises(ValueError, match="keeps no normals"):
        kept.kept_normals()
    agree("after drop_normals")
    for c in clouds:
        c.insert(moved[:50])
    agree("and an edit without kept normals")
    plain.close()


def test_registration_with_other_parameters_leaves_the_kept_rows(gpu_ctx):
    m = pkg()
    other = m.Context(0)
    rows = G.corner_rows()
    src = f32(G.moved_back(G.corner_source(500, 500), G.KNOWN))
    kept, plain = (m.voxel_downsample(rows, H, context=ctx) for ctx in (gpu_ctx, other))
    kept.keep_normals(2 * H, 30)
    before = kept.kept_normals()
    for kw in (dict(normals_radius=1.5 * H), dict(max_nn=12), dict(normals_radius=np.nextafter(2 * H, 1.0)), dict(max_nn=0)):
        a, b = (reg_raw(c.register(src, 2 * H, max_iterations=3, **kw)) for c in (kept, plain))
        assert a == b, kw
        assert raw(kept.kept_normals()) == raw(before) and kept.kept.full_passes == 1, kw
    plain.close()


# ---- lifetime ----------------------------------------------------------------------------------------------------------------
def test_keeping_again_replaces_and_a_new_build_ends(gpu_ctx):
    m = pkg()
    rows = K.sheet(500, seed=60, h=H)
    cloud = m.voxel_downsample(rows, H, context=gpu_ctx)
    assert cloud.kept is None
    with pytest.raises(ValueError, match="keeps no normals"):
        cloud.kept_normals()
    cloud.keep_normals(H, 0)
    assert raw(cloud.kept_normals()) == raw(cloud.normals(H, 0))
    cloud.keep_normals(3 * H, 5)
    k = cloud.kept
    assert (k.radius, k.max_nn, k.full_passes, k.refreshed_last) == (3 * H, 5, 2, 0)
    assert raw(cloud.kept_normals()) == raw(cloud.normals(3 * H, 5))
    cloud.insert(rows[:10])
    assert cloud.kept.refreshed_last > 0 and raw(cloud.kept_normals()) == raw(cloud.normals(3 * H, 5))
    with pytest.raises(ValueError):
        cloud.keep_normals(5 * H)                                # refused: what was kept stays
    assert cloud.kept.radius == 3 * H
    again = m.voxel_downsample(rows, H, context=gpu_ctx)
    assert again.kept is None
    with pytest.raises(ValueError, match="closed or was replaced"):
        cloud.kept_normals()
    again.keep_normals()
    assert again.kept.full_passes == 1 and again.kept.refreshed_total == 0
    t = gpu_ctx.read_timing_kept_normals()
    assert set(t) >= {"mark_ms", "window_ms", "cap_ms", "carry_ms"}
