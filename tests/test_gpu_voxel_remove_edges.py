"""Shrinking a voxel cloud on the device where tests/test_gpu_voxel_remove.py stops short (builders and their conditions:
tests/voxelremoveedges.py, asserted in tests/test_voxel_remove_edges_cpu.py): removals past 256 workgroups of voxels and
the shrink rule's edge there, a mixed insert into a table refilled in place, records past one workgroup and one pass, a
point total past 32 bits, holes inside probe chains that wrap, refusals that undo thousands of items, sums past 2^53,
the 910 frames, wide rows, a time column and the fuzz grids as subtracted sources, a sliding window, and what a shrunk
cloud invalidates.  Every comparison is exact and with the NumPy restatements of tests/voxelremove.py, voxelinsert.py
and voxel.py, and where the definition says so with a fresh voxel_downsample of what is left; a refusal is held to the
item it names, to the library's ``why`` code and to a cloud unchanged in everything it gives out."""
import collections
import ctypes

import numpy as np
import pytest

import registration as R
import voxel as V
import voxeledges as E
import voxelinsert as VI
import voxelinsertedges as IE
import voxelremove as VR
import voxelremoveedges as RE
from conftest import pkg
from test_gpu_voxel_remove import analyses, as_batch, bits, check, emits, same_emits, same_results, table

pytestmark = pytest.mark.gpu


def state_of(rec, h, origin=V.ZERO):
    """Restatement records (keys, n, S, SI) as the VoxelSums a merge or a subtraction takes."""
    keys, n, S, SI = rec
    return pkg().VoxelSums(np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(n, dtype=np.int32),
                           np.ascontiguousarray(np.column_stack([S, SI]), dtype=np.int64), float(h), np.array(origin, np.float64))


def state_of_rows(rows, h, origin=V.ZERO):
    return state_of(VI.records_of(V.downsample(rows, h, origin)), h, origin)


def build(ctx, rows, h, origin=V.ZERO):
    """The cloud of rows on the device and restated."""
    cloud, want = pkg().voxel_downsample(rows, h, origin, context=ctx), VR.Cloud(h, origin)
    want.insert(rows)
    return cloud, want


def by_key(keys):
    return np.argsort(V.pack(keys), kind="stable")


def same_records_by_key(got, fresh, what):
    """The emits of a cloud against V.downsample's dict of the rows left, which may number the voxels differently."""
    a, b = by_key(got["keys"]), by_key(fresh["keys"])
    assert np.array_equal(got["keys"][a], fresh["keys"][b]) and np.array_equal(got["counts"][a], fresh["counts"][b]), what
    assert np.array_equal(got["sums"][a], np.column_stack([fresh["S"], fresh["SI"]])[b]), what
    assert np.array_equal(bits(got["rows"][a]), bits(fresh["rows"][b])), what
    assert np.array_equal(bits(got["f32"][a]), bits(fresh["f32"][b])), what


def raw_subtract(ctx, src):
    """mc_voxel_subtract_* at the C entry -> (its return value, voxels emptied, the item it names, its why code); the
    item is a row or record index, or (frame, point) for a batch, -1 where none is named."""
    gone, item, frame, why = ctypes.c_int64(7), ctypes.c_int64(7), ctypes.c_int32(7), ctypes.c_int32(7)
    out = (ctypes.byref(gone), ctypes.byref(item), ctypes.byref(why))
    bufs = []

    def device(a):
        a = np.ascontiguousarray(a)
        bufs.append(ctx.device_buffer(max(a.nbytes, 8)))
        bufs[-1].from_host(a)
        return bufs[-1].ptr
    try:
        if hasattr(src, "sums"):
            rc = ctx.lib.mc_voxel_subtract_sums(ctx.handle, device(src.keys), device(src.counts), device(src.sums), len(src.keys), *out)
        elif hasattr(src, "handle"):
            rc = ctx.lib.mc_voxel_subtract_batch(ctx.handle, src.handle, out[0], ctypes.byref(frame), out[1], out[2])
            return rc, gone.value, (frame.value, item.value) if frame.value >= 0 else -1, why.value
        else:
            rows = np.ascontiguousarray(src, dtype=np.float64)
            rc = ctx.lib.mc_voxel_subtract_f64(ctx.handle, device(rows), rows.shape[1], len(rows), *out)
        return rc, gone.value, item.value, why.value
    finally:
        for b in bufs:
            b.close()


def refused(ctx, cloud, before, src, item, reason, match, slots=None):
    """A refused subtraction: the library names ``item`` and gives ``reason``'s why code, the wrapper raises a message
    that matches, and the cloud gives out what it gave before."""
    assert raw_subtract(ctx, src) == (pkg()._lib.MC_ERR_INVALID, 0, item, VR.WHY[reason]), match
    with pytest.raises(ValueError, match=match):
        cloud.subtract(src)
    same_emits(emits(cloud), before, match)
    assert slots is None or table(ctx) == slots, match


def restated_refusal(call):
    with pytest.raises(V.Refused) as e:
        call()
    return e.value.index, e.value.reason, e.value.key


# ---- A: past 256 workgroups of voxels --------------------------------------------------------------------------------
@pytest.mark.parametrize("M,name", RE.MANY_CASES)
def test_a_removal_past_256_workgroups_of_voxels(gpu_ctx, M, name):
    """256, 257 and 514 workgroups of voxels: the selection scan of compact() takes a second and a third pass,
    k_vox_keep, k_vox_compact and k_vox_refill run a tail workgroup, and vox_block_add sums the survivors' points over
    all of them into one word, which n_points reports."""
    ctx, h = gpu_ctx, RE.MANY_H
    rows = RE.many_voxels(M)
    mask = RE.masks(M)[name]
    cloud, want = build(ctx, rows, h)
    tab = RE.Table(len(rows))
    assert cloud.n_voxels == M and table(ctx) == tab.now()
    gone = V.pack(want.keys[mask])
    assert cloud.remove(mask) == want.remove(mask) == int(mask.sum()), name
    assert table(ctx) == tab.kept(M, M - int(mask.sum())), name
    got = check(cloud, want.result(), name)
    left = rows[~np.isin(RE.packed(rows, h), gone)]
    assert cloud.n_points == len(left) == 2 * (M - int(mask.sum())), name
    fresh = pkg().voxel_downsample(left, h, context=ctx)
    same_emits(got, emits(fresh), (name, "fresh"))


@pytest.mark.parametrize("which", [0, 1])
def test_the_shrink_edge_at_65537_voxels_and_a_mixed_insert(gpu_ctx, which):
    """Exactly an eighth of the slots in survivors keeps the table, which k_vox_refill then fills in place; one fewer
    shrinks it.  Either way an insert of survivors' keys, leavers' keys and new keys finds the table as a build would
    have left it: occupied slots hold a first index of the cloud, empty ones none."""
    ctx, h = gpu_ctx, RE.MANY_H
    slots, stay, one_fewer = RE.shrink_edge()
    keep = (stay, one_fewer)[which]
    rows, mask, mixed = RE.many_voxels(RE.EDGE_M), RE.edge_mask(keep), RE.mixed_rows(keep)
    cloud, want = build(ctx, rows, h)
    tab = RE.Table(len(rows))
    assert table(ctx) == tab.now() == (slots, 0)
    assert cloud.remove(mask) == want.remove(mask) == RE.EDGE_M - keep
    after = 1 << VR.table_shrink_log2(keep, slots.bit_length() - 1)
    assert table(ctx) == tab.kept(RE.EDGE_M, keep) == (after, 0) and (after == slots) == (which == 0)
    check(cloud, want.result(), ("kept", keep))
    grown = want.insert(mixed)
    assert cloud.insert(as_batch(ctx, [1000, 0, 2000], mixed) if which else mixed) == grown
    assert table(ctx) == tab.call(keep, len(mixed)) == (after, 0)
    got = check(cloud, want.result(), ("mixed insert", keep), n_points=2 * keep + len(mixed))
    # the voxels that left are new ids again, behind the survivors, and what is there is a fresh build of the sources
    leavers = V.pack(RE.own_keys(np.flatnonzero(mask)))
    left = rows[~np.isin(RE.packed(rows, h), leavers)]
    ids = dict(zip(V.pack(got["keys"]).tolist(), range(cloud.n_voxels)))
    assert all(ids[key] >= keep for key in leavers.tolist())
    same_emits(got, emits(pkg().voxel_downsample(np.concatenate([left, mixed]), h, context=ctx)), "fresh")


# ---- B: records past one workgroup and one scan pass -----------------------------------------------------------------
@pytest.mark.parametrize("m", RE.RECORD_COUNTS)
def test_merged_records_subtracted_in_another_order(gpu_ctx, m):
    """2047, 2048, 2049 and 4097 records: k_vox_sub_validate<records> with a tail in its last round, exactly one
    workgroup, and a second and third workgroup that hold one record."""
    ctx, h = gpu_ctx, RE.MANY_H
    rows, rec, again = RE.record_identity_case(m)
    cloud, want = build(ctx, rows, h)
    tab = RE.Table(len(rows))
    before = emits(cloud)
    grown = want.merge(*rec)
    assert cloud.merge(state_of(rec, h)) == grown and table(ctx) == tab.call(len(rows), m)
    check(cloud, want.result(), ("merged", m), n_points=len(rows) + m)
    assert cloud.subtract(state_of(again, h)) == grown == want.subtract_records(*again)
    assert table(ctx) == tab.kept(len(rows) + grown, len(rows))
    same_emits(emits(cloud), before, m)
    check(cloud, want.result(), ("and taken out", m), n_points=len(rows))


def test_records_past_one_pass_as_a_subtraction(gpu_ctx):
    """610 308 records in 299 workgroups of 2048: every workgroup adds its points into meta[2..3], the refused record
    of the second pass is the lower of two and of either kind, and the accepted call gives the head's cloud back."""
    ctx = gpu_ctx
    head, h, rec = IE.records_case()
    M, grown, merged, N = IE.records_want()
    m = len(rec[0])
    cloud = pkg().voxel_downsample(head, h, context=ctx)
    try:
        tab = RE.Table(len(head))
        head_emits = emits(cloud)
        assert cloud.merge(state_of(rec, h)) == grown and table(ctx) == tab.call(M, m)
        before = check(cloud, merged, "merged", n_points=N)
        refused(ctx, cloud, before, state_of(IE.refused_records(), h), IE.RECORDS_BAD, VR.ITEM,
                rf"record {IE.RECORDS_BAD} .*a count below 1", tab.now())
        refused(ctx, cloud, before, state_of(RE.records_missing(), h), IE.RECORDS_BAD, VR.MISSING,
                rf"record {IE.RECORDS_BAD} .*holds no voxel", tab.now())
        assert cloud.n_points == N and cloud.n_voxels == M + grown
        assert cloud.subtract(state_of(RE.records_again(), h)) == grown
        assert table(ctx) == tab.kept(M + grown, M)
        same_emits(emits(cloud), head_emits, "the head's cloud")
        check(cloud, V.downsample(head, h), "the head's cloud, restated", n_points=len(head))
    finally:
        cloud.close()


def test_a_point_total_past_32_bits_is_refused_for_the_points(gpu_ctx):
    """Four records of 2^30 points: the host reads meta[2..3] as one 64-bit total, 4 294 967 296; its low word is 0."""
    ctx = gpu_ctx
    cloud, want = build(ctx, RE.POINTS_ROWS, RE.POINTS_H)
    before, slots = emits(cloud), table(ctx)
    assert restated_refusal(lambda: want.subtract_records(*RE.POINTS_CASE)) == (-1, VR.POINTS, None)
    refused(ctx, cloud, before, state_of(RE.POINTS_CASE, RE.POINTS_H), -1, VR.POINTS, RE.POINTS_MESSAGE, slots)
    assert cloud.n_points == 3 and cloud.n_voxels == 1
    check(cloud, want.result(), "unchanged", n_points=3)
    # and one such record less its points is no set of points: the count fits, the voxel does not hold them
    one = tuple(a[:1] for a in RE.POINTS_CASE)
    assert restated_refusal(lambda: want.subtract_records(*one))[:2] == (-1, VR.POINTS)
    refused(ctx, cloud, before, state_of(one, RE.POINTS_H), -1, VR.POINTS, r"brings 1073741824 points and the cloud holds 3", slots)


# ---- C: holes inside chains ------------------------------------------------------------------------------------------
def finds_every_key(ctx, cloud, want, what):
    """A subtraction of one point of every voxel held and then a row of NaN: the lookup of k_vox_sub_validate finds
    every key through the chains as they are, so the NaN, the last item, is the lowest refused; nothing changes."""
    res = want.result()
    rows = np.concatenate([res["rows"], [[np.nan, 0.0, 0.0, 0.0]]])
    assert restated_refusal(lambda: want.subtract(rows))[:2] == (len(rows) - 1, VR.ITEM), what
    assert raw_subtract(ctx, rows) == (pkg()._lib.MC_ERR_INVALID, 0, len(rows) - 1, VR.WHY[VR.ITEM]), what


def run_plan(ctx, cloud, h, steps, done, what):
    """The calls of a plan on the device: after every one the cloud is the restatement's, the table is the rules',
    and every key held is found."""
    for k, ((kind, arg), (out, want, at, _, _)) in enumerate(zip(steps, done)):
        got = cloud.remove(np.array(arg)) if kind == "remove" else cloud.subtract(arg) if kind == "subtract" else cloud.insert(arg)
        assert got == out and table(ctx) == at, (what, k)
        N = int(want["counts"].sum())
        check(cloud, want, (what, k), n_points=N)
        if len(want["keys"]):
            held = VR.Cloud(h)
            held.keys, held.n, held.S, held.SI, held.N = (want["keys"].astype(np.int64), want["counts"].astype(np.int64), want["S"],
                                                          want["SI"], N)
            finds_every_key(ctx, cloud, held, (what, k))
            check(cloud, want, (what, k, "after the lookup"), n_points=N)
    return cloud


def test_holes_inside_chains_that_wrap(gpu_ctx):
    """6167 keys that start in the last 2^-12 * 96 of every table, grown as voxelinsertedges.live_chain_case grows them;
    then a third of them leaves and the table is refilled in place, a subtraction empties more, every key is inserted
    again, and removals take the cloud down to 2000, 100 and 3 voxels through three smaller tables before the chain
    comes back.  A refill that loses a key behind a hole, or a lookup that stops at one, shows as MISSING."""
    ctx, mc, h = gpu_ctx, pkg(), IE.CHAIN_H
    _, grow = IE.live_chain_case()
    cloud = None
    for kind, rows, counts in grow:
        if kind == "build":
            cloud = mc.voxel_downsample(rows, h, context=ctx)
        elif kind == "records":
            cloud.merge(state_of(IE.point_records(rows, h), h))
        else:
            cloud.insert(as_batch(ctx, counts, rows) if kind == "batch" else rows)
    assert table(ctx) == IE.LIVE_CHAIN_TABLES[-1] and cloud.n_voxels == 6167
    steps, done = RE.chain_plan()
    run_plan(ctx, cloud, h, steps, done, "chain")
    assert cloud.n_voxels == 6167


def test_the_minimum_table_under_removals(gpu_ctx):
    """65 colliding keys in 256 slots down to 7, 1 and 0 voxels: the 64-slot floor each time, and the rows again."""
    ctx = gpu_ctx
    _, parts, h = IE.min_table_case()
    cloud = pkg().voxel_downsample(np.zeros((0, 4)), h, context=ctx)
    for rows in parts:
        cloud.insert(rows)
    assert table(ctx) == IE.MIN_TABLES[-1]
    steps, done, _ = RE.min_table_plan()
    run_plan(ctx, cloud, h, steps, done, "64 slots")
    assert cloud.n_voxels == 65 and cloud.n_points == 65


# ---- D: refusals that must undo much ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rows", "batch"])
def test_a_refusal_that_undoes_thousands_of_items(gpu_ctx, kind):
    """40 voxels over-drawn by a point, 50 emptied exactly and 800 left with one point in one call of 5237 items: the
    counts of the 40 wrap below 0, k_vox_sub_check names the lowest item of any of them, k_vox_sub_apply(+1) brings every
    record back, and nothing compacts although 50 voxels stood at 0.  Without the 40 points the call is accepted."""
    ctx, h = gpu_ctx, RE.SOURCE_H
    call, accepted, counts, counts_ok = RE.overdrawn_case()
    cloud, want = build(ctx, RE.source(), h)
    before, slots = emits(cloud), table(ctx)
    index, reason, key = restated_refusal(lambda: want.subtract(call))
    assert reason == VR.REMAINDER
    if kind == "batch":
        off = np.concatenate([[0], np.cumsum(counts)])
        f = int(np.searchsorted(off, index, side="right")) - 1
        item, name, src, ok = (f, index - int(off[f])), f"frame {f}, point {index - int(off[f])} ", as_batch(ctx, counts, call), \
            as_batch(ctx, counts_ok, accepted)
    else:
        item, name, src, ok = index, f"row {index} ", call, accepted
    refused(ctx, cloud, before, src, item, VR.REMAINDER, name + r".*voxel \(%d, %d, %d\) .*no set of points" % key, slots)
    assert cloud.n_points == 6000 and cloud.n_voxels == len(before["keys"])
    check(cloud, want.result(), "unchanged", n_points=6000)
    emptied = want.subtract(accepted)
    assert cloud.subtract(ok) == emptied == RE.OVERDRAWN + RE.EMPTIED
    got = check(cloud, want.result(), "accepted", n_points=6000 - len(accepted))
    assert (got["counts"] == 1).all() and table(ctx) == RE.Table(6000).kept(len(before["keys"]), cloud.n_voxels)


def test_every_item_refused_and_two_kinds_far_apart(gpu_ctx):
    """Every lane of 20 workgroups has an item for vox_lowest's word; and the lower of a NaN and a point off the cloud,
    in the first and the last workgroup, decides the kind whichever word of meta holds it."""
    ctx, h = gpu_ctx, RE.SOURCE_H
    cloud, want = build(ctx, RE.source(), h)
    before, slots = emits(cloud), table(ctx)
    nan, off = RE.all_bad_rows()
    assert restated_refusal(lambda: want.subtract(nan))[:2] == (0, VR.ITEM)
    refused(ctx, cloud, before, nan, 0, VR.ITEM, r"row 0 .*not finite", slots)
    assert restated_refusal(lambda: want.subtract(off))[:2] == (1, VR.MISSING)
    refused(ctx, cloud, before, off, 1, VR.MISSING, r"row 1 .*holds no voxel", slots)
    refused(ctx, cloud, before, as_batch(ctx, [0, 2, 4998], off), (1, 1), VR.MISSING, r"frame 1, point 1 .*holds no voxel", slots)
    for rows, index, reason in RE.far_apart_cases():
        assert restated_refusal(lambda: want.subtract(rows))[:2] == (index, reason)
        match = r".*not finite" if reason == VR.ITEM else r".*holds no voxel"
        refused(ctx, cloud, before, rows, index, reason, rf"row {index} " + match, slots)
        refused(ctx, cloud, before, as_batch(ctx, [2, 0, 4998], rows), (2, index - 2), reason, rf"frame 2, point {index - 2} " + match, slots)
    check(cloud, want.result(), "unchanged", n_points=6000)


def test_refused_subtractions_are_named_among_empty_frames(gpu_ctx):
    """voxelinsertedges.refusal_cases on the 910-frame batch, subtracted from the cloud that holds it."""
    ctx = gpu_ctx
    counts = E.frame_run_counts()
    good, _ = E.frame_run_rows(False)
    held, h = RE.frame_cloud()
    cloud, want = build(ctx, held, h)
    before, slots = check(cloud, want.result(), "built", n_points=len(held)), table(ctx)
    for what, at, (f, i, dense) in IE.refusal_cases():
        rows = IE.refused_rows(good, at)
        assert restated_refusal(lambda: want.subtract(rows))[:2] == (dense, VR.ITEM), what
        refused(ctx, cloud, before, as_batch(ctx, counts, rows), (f, i), VR.ITEM, rf"frame {f}, point {i} ", slots)
        refused(ctx, cloud, before, rows, dense, VR.ITEM, rf"row {dense} ", slots)
    # and the cloud still gives the batch up
    assert cloud.subtract(as_batch(ctx, counts, good)) == want.subtract(good)
    check(cloud, V.downsample(IE.other_points(), h), "the good batch after nine refusals", n_points=len(IE.other_points()))


# ---- E: sums past 2^53 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rows", "records"])
def test_sums_past_2_53_come_out_exactly(gpu_ctx, kind):
    """Two voxels of 2 200 001 points, sums past 2^53 and odd, less all but the last point of each: what is left is
    that point's own quantities.  The rows variant uploads and subtracts 4.4 million rows: the slowest test here."""
    ctx = gpu_ctx
    rows, h, o = E.big_sum_case()
    head, last, off = RE.big_records()
    cloud = pkg().voxel_downsample(rows, h, o, context=ctx)
    try:
        slots = table(ctx)
        assert cloud.subtract(rows[:-2] if kind == "rows" else state_of(head, h, o)) == 0
        before = check(cloud, last, kind, n_points=2)
        assert table(ctx) == slots                                  # no voxel emptied: the table is the build's
        if kind == "records":
            refused(ctx, cloud, before, state_of(off, h, o), 0, VR.REMAINDER, r"record 0 .*voxel \(0, 0, 0\) .*no set of points", slots)
        assert cloud.subtract(rows[-2:]) == 2 and cloud.n_voxels == 0 == cloud.n_points
        assert table(ctx) == RE.Table(len(rows)).kept(2, 0)
        cloud = pkg().voxel_downsample(rows[-2:], h, o, context=ctx)
        same_emits(before, emits(cloud), "fresh")
    finally:
        cloud.close()


# ---- F: layouts and grids --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_voxel", [True, False])
def test_frame_runs_as_a_subtracted_source(gpu_ctx, one_voxel):
    ctx = gpu_ctx
    rows, h = E.frame_run_rows(one_voxel)
    other = IE.other_points()
    (c0, a0, b0), (c1, a1, b1) = IE.frame_halves()
    cloud, want = build(ctx, other, h)
    for c, a, b in ((c0, a0, b0), (c1, a1, b1)):
        assert cloud.insert(as_batch(ctx, c, rows[a:b])) == want.insert(rows[a:b])
    assert cloud.subtract(as_batch(ctx, c0, rows[a0:b0])) == want.subtract(rows[a0:b0])
    got = check(cloud, want.result(), (one_voxel, "less the first half"), n_points=len(other) + b1 - a1)
    same_records_by_key(got, V.downsample(np.concatenate([other, rows[a1:b1]]), h), one_voxel)
    fresh = emits(pkg().voxel_downsample(np.concatenate([other, rows[a1:b1]]), h, context=ctx))
    a, b = by_key(got["keys"]), by_key(fresh["keys"])
    for f in ("keys", "counts", "rows", "f32", "sums"):
        assert got[f][a].tobytes() == fresh[f][b].tobytes(), (one_voxel, f)
    cloud, want = build(ctx, np.concatenate([other, rows]), h)
    assert cloud.subtract(as_batch(ctx, c0, rows[a0:b0])) == want.subtract(rows[a0:b0])
    check(cloud, want.result(), (one_voxel, "the whole less the first half"))
    assert cloud.subtract(as_batch(ctx, c1, rows[a1:b1])) == want.subtract(rows[a1:b1])
    check(cloud, V.downsample(other, h), (one_voxel, "less both"), n_points=len(other))


@pytest.mark.parametrize("ld", [6, 7])
def test_wide_rows_as_a_subtracted_source(gpu_ctx, ld):
    ctx = gpu_ctx
    h, o = IE.WIDE_GRID
    rows = IE.wide_rows(ld)
    four = np.ascontiguousarray(rows[:, :4])
    cloud, want = build(ctx, four, h, o)
    gone = want.subtract(four[:IE.WIDE_CUT])
    assert cloud.subtract(rows[:IE.WIDE_CUT]) == gone > 0
    wide = check(cloud, want.result(), f"rows of {ld} columns", n_points=len(rows) - IE.WIDE_CUT)
    same_records_by_key(wide, V.downsample(four[IE.WIDE_CUT:], h, o), ld)
    cloud = pkg().voxel_downsample(rows, h, o, context=ctx)
    assert cloud.subtract(four[:IE.WIDE_CUT]) == gone
    same_emits(emits(cloud), wide, "the same points in four columns")
    left = cloud.n_voxels
    assert cloud.subtract(rows[IE.WIDE_CUT:]) == left == want.subtract(four[IE.WIDE_CUT:]) and cloud.n_points == 0 == cloud.n_voxels


def test_a_batch_with_a_time_column_as_a_subtracted_source(gpu_ctx):
    ctx = gpu_ctx
    rows, times, h = IE.timed_case()
    seen = {}
    for with_time in (True, False):
        cloud, want, a = *build(ctx, rows, h), 0
        for c in IE.TIMED_COUNTS:
            part = rows[a:a + sum(c)]
            b = ctx.batch(c, with_time=with_time)
            b.upload_columns(*[part[:, k].astype(np.float32) for k in range(4)])
            if with_time:
                b.upload_time(times[a:a + sum(c)])
            assert b.with_time == with_time
            a += sum(c)
            assert cloud.subtract(b) == want.subtract(part)
            seen[with_time, a] = check(cloud, want.result(), (with_time, a), n_points=len(rows) - a)
            if a < len(rows):
                same_records_by_key(seen[with_time, a], V.downsample(rows[a:], h), with_time)
        assert cloud.n_voxels == 0
    for (with_time, a), got in seen.items():
        same_emits(got, seen[not with_time, a])


@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_grid_fuzz_taken_apart_in_reverse(gpu_ctx, seed):
    ctx = gpu_ctx
    h, o, _, rows32 = E.fuzz_case(seed)
    what = f"fuzz {seed}: h {h}, origin {o}"
    tail = [rows32[:1000], rows32[1000:]]
    for kind, parts in (("rows", IE.fuzz_parts(rows32, IE.FUZZ_ROW_CUTS)), ("batches", tail)):
        cloud, want = build(ctx, rows32, h, o)
        for k in range(len(parts) - 1, -1, -1):
            src = as_batch(ctx, IE.FUZZ_BATCHES[k], parts[k]) if kind == "batches" else parts[k]
            assert cloud.subtract(src) == want.subtract(parts[k]), (what, kind, k)
            check(cloud, want.result(), (what, kind, k), n_points=sum(len(p) for p in parts[:k]))
            if k:
                check(cloud, V.downsample(np.concatenate(parts[:k]), h, o), (what, kind, k, "the rows left"))
        assert cloud.n_voxels == 0 == cloud.n_points
        assert cloud.insert(parts[0]) == want.insert(parts[0])
        got = check(cloud, V.downsample(parts[0], h, o), (what, kind, "part 0 again"), n_points=len(parts[0]))
        same_emits(got, emits(pkg().voxel_downsample(parts[0], h, o, context=ctx)), (what, kind, "fresh"))


# ---- G: a sliding window ---------------------------------------------------------------------------------------------
def test_a_sliding_window_forgets_what_it_inserted_first(gpu_ctx):
    """40 frames of 2000 points through a window of five: insert frame i, subtract frame i - 5, as rows, as a batch
    with an empty frame and as a state in turn."""
    ctx = gpu_ctx
    frames, h = RE.window_case()
    steps = RE.window_want()
    cloud = pkg().voxel_downsample(np.zeros((0, 4)), h, context=ctx)

    def source(f, kind):
        return frames[f] if kind == "rows" else as_batch(ctx, RE.WINDOW_COUNTS, frames[f]) if kind == "batch" else state_of_rows(frames[f], h)
    for i, (grown, gone, want, at, N) in enumerate(steps):
        kind = RE.WINDOW_KINDS[i % 3]
        src = source(i, kind)
        assert (cloud.merge(src) if kind == "state" else cloud.insert(src)) == grown, i
        if gone is not None:
            assert cloud.subtract(source(i - RE.WINDOW, kind)) == gone, i
        assert cloud.n_points == N, i
        if want is not None:
            assert table(ctx) == at, i
            got = check(cloud, want, ("window", i), n_points=N)
    same_records_by_key(got, V.downsample(np.concatenate(frames[35:]), h), "frames 35..39")
    assert cloud.n_points == 10000


# ---- H: what a shrunk cloud invalidates ------------------------------------------------------------------------------
Selected = collections.namedtuple("Selected", "cols")
MASK_MESSAGE = r"must be a bool array of shape \({M},\)"


def everything(ctx, cloud, src, mask, h):
    """test_gpu_voxel_remove's analyses and the ones it leaves out: one registration per frame of a three-frame
    source, a selection, and a plane among a mask."""
    frames = as_batch(ctx, [400, 0, 600], np.column_stack([src, np.zeros(len(src))]))
    cols = np.stack(cloud.select(mask).download_columns(), axis=1)
    return dict(analyses(cloud, src, h), frames=cloud.register_frames(frames, 2 * h), selected=Selected(cols),
                among=cloud.segment_plane(h, 200, among=mask))


def test_every_analysis_after_a_removal_and_after_a_subtraction(gpu_ctx):
    ctx, mc, h = gpu_ctx, pkg(), R.H
    STATE = mc._lib.MC_ERR_STATE
    rows = R.corner_rows()
    src = R.moved_back(R.corner_source(1000, 3), R.NEARBY)
    cloud = mc.voxel_downsample(rows, h, context=ctx)
    M = cloud.n_voxels
    old_mask = IE.corner_mask(M)
    stale = everything(ctx, cloud, src, old_mask, h)               # clusters, their statistics, normals, registrations
    plane = stale["plane"]
    gone = V.pack(cloud.keys()[plane.inliers])
    assert 200 <= plane.n_inliers < M and cloud.remove(plane.inliers) == plane.n_inliers
    Mk = M - plane.n_inliers
    mask = IE.corner_mask(Mk)
    # the statistics of the clustering before are gone with it
    K = stale["clusters"].n_clusters
    assert K >= 1
    buf = ctx.device_buffer(36 * K)
    try:
        base = buf.ptr.value
        assert ctx.lib.mc_voxel_cluster_stats(ctx.handle, base + 8 * K, base, base + 12 * K, base + 24 * K) == STATE
    finally:
        buf.close()
    # a mask of the old length is refused and changes nothing
    shrunk = emits(cloud)
    for call in (lambda: cloud.segment_plane(h, 200, among=old_mask), lambda: cloud.remove(old_mask), lambda: cloud.select(old_mask)):
        with pytest.raises(ValueError, match=MASK_MESSAGE.format(M=Mk)):
            call()
    same_emits(emits(cloud), shrunk, "old masks")
    got = everything(ctx, cloud, src, mask, h)
    left = rows[~np.isin(RE.packed(rows, h), gone)]
    fresh = mc.voxel_downsample(left, h, context=ctx)
    same_emits(shrunk, emits(fresh), "fresh")
    want = everything(ctx, fresh, src, mask, h)
    same_results(got, want)
    assert want["clusters"].n_clusters >= 1 and want["register"].pairs > 100 and len(want["normals"].normals) == Mk
    assert want["frames"].status_names[1] == "empty" and (want["frames"].pairs[[0, 2]] > 50).all()
    assert len(want["selected"].cols) == mask.sum() and want["among"].n_inliers >= 100 and not (want["among"].inliers & ~mask).any()

    # a subtraction that empties no voxel: the ids stay, the centroids move, and every analysis is computed again
    take, far = RE.moved_centroid_case()
    cloud = mc.voxel_downsample(rows, h, context=ctx)
    keys, cent = cloud.keys(), cloud.rows()
    mask = IE.corner_mask(M)
    stale = everything(ctx, cloud, src, mask, h)
    assert cloud.subtract(take) == 0 and np.array_equal(cloud.keys(), keys)
    assert np.abs(cloud.rows()[far, :3] - cent[far, :3]).max() > h / 10
    got_cloud, got = emits(cloud), everything(ctx, cloud, src, mask, h)
    # a one-shot build of the rows left, sorted by voxel id so that it numbers the voxels alike
    vid = np.searchsorted(np.sort(V.pack(keys)), RE.packed(rows, h))
    vid = by_key(keys)[vid]
    keep = ~(rows[:, None, :] == take[None, :, :]).all(axis=2).any(axis=1)
    left = rows[keep][np.argsort(vid[keep], kind="stable")]
    assert len(left) == len(rows) - len(take)
    fresh = mc.voxel_downsample(left, h, context=ctx)
    same_emits(got_cloud, emits(fresh), "fresh, in the cloud's order")
    want = everything(ctx, fresh, src, mask, h)
    same_results(got, want)
    # and they are not what they were: the clusters hold fewer points, the source's nearest centroids have moved
    assert got["clusters"].points.tobytes() != stale["clusters"].points.tobytes()
    assert got["nearest"].dist2.tobytes() != stale["nearest"].dist2.tobytes()
