"""The edge cases of a shrinking voxel cloud without a GPU: every builder of tests/voxelremoveedges.py holds the
condition that makes its case bite (tests/test_gpu_voxel_remove_edges.py runs the same cases on the kernels), checked on
the NumPy restatements of tests/voxel.py, voxelinsert.py and voxelremove.py alone; every table size comes from
voxelinsert.table_log2 and voxelremove.table_shrink_log2."""
import numpy as np
import pytest

import registration as R
import voxel as V
import voxeledges as E
import voxelinsert as VI
import voxelinsertedges as IE
import voxelremove as VR
import voxelremoveedges as RE

FIELDS = ("rows", "counts", "keys", "f32", "S", "SI")


def same_cloud(a, b, order=None):
    """Two restatement results (or V.downsample's dicts), every field to the bit; order: (of a, of b)."""
    for f in FIELDS:
        x, y = (a[f], b[f]) if order is None else (a[f][order[0]], b[f][order[1]])
        assert x.dtype == y.dtype and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), f


def by_key(d):
    return np.argsort(V.pack(d["keys"]), kind="stable")


def cloud_of(rows, h, origin=V.ZERO):
    c = VR.Cloud(h, origin)
    c.insert(rows)
    return c


def refusal(call):
    with pytest.raises(V.Refused) as e:
        call()
    return e.value.index, e.value.reason, e.value.key


# ---- A ---------------------------------------------------------------------------------------------------------------
def test_many_voxels_are_more_than_one_scan_pass_of_workgroups():
    assert [-(-M // RE.BLOCK) for M in RE.MANY] == [256, 257, 514] and RE.MANY[0] % RE.BLOCK == 0
    assert all(M % RE.BLOCK for M in RE.MANY[1:])
    assert [-(-(-(-M // RE.BLOCK)) // RE.SCAN_PASS) for M in RE.MANY] == [1, 2, 3]      # passes of the selection scan
    assert len(RE.MANY_CASES) == 8 * 3 - 1
    for M in RE.MANY:
        rows = RE.many_voxels(M)
        d = V.downsample(rows, RE.MANY_H)
        assert len(rows) == 2 * M and len(d["keys"]) == M and (d["counts"] == 2).all()
        assert np.array_equal(d["keys"], RE.own_keys(np.arange(M)))                       # voxel ids are voxel numbers
        vox = RE.packed(rows, RE.MANY_H)
        for name, mask in RE.masks(M).items():
            assert (M, name) in RE.MANY_CASES and mask.dtype == np.bool_ and mask.shape == (M,)
            want = cloud_of(rows, RE.MANY_H)
            assert want.remove(mask) == mask.sum()
            left = rows[~np.isin(vox, V.pack(d["keys"][mask]))]
            assert want.N == len(left) == 2 * (M - mask.sum())
            same_cloud(want.result(), V.downsample(left, RE.MANY_H))
        m = RE.masks(M)
        assert m["alternate"].sum() == (M + 1) // 2 and m["all but voxel 40000"].sum() == M - 1
        assert m["everything from 65536 on"].sum() == M - 65536 and 0.09 * M < m["a seeded tenth"].sum() < 0.11 * M
        # the single voxels lie in the first and the last workgroup, and on either side of the scan's pass boundary
        assert np.flatnonzero(m["only voxel 65535"])[0] // RE.BLOCK == RE.SCAN_PASS - 1
        if M > 65536:
            assert np.flatnonzero(m["only voxel 65536"])[0] // RE.BLOCK == RE.SCAN_PASS


def test_the_shrink_edge_at_65537_voxels_and_the_mixed_insert():
    slots, stay, one_fewer = RE.shrink_edge()
    log2cap = E.table_log2(2 * RE.EDGE_M)
    assert slots == 1 << log2cap and RE.EDGE_M > stay == slots // 8 and one_fewer == stay - 1
    assert VR.table_shrink_log2(stay, log2cap) == log2cap
    shrunk = VR.table_shrink_log2(one_fewer, log2cap)
    assert shrunk < log2cap and (1 << shrunk) >= 4 * one_fewer > (1 << (shrunk - 1))
    rows = RE.many_voxels(RE.EDGE_M)
    for keep, after in ((stay, log2cap), (one_fewer, shrunk)):
        mask = RE.edge_mask(keep)
        assert (~mask).sum() == keep and mask[:65536].any()
        table = RE.Table(len(rows))
        assert table.kept(RE.EDGE_M, keep) == (1 << after, 0)
        want = cloud_of(rows, RE.MANY_H)
        gone = V.pack(want.keys[mask])
        want.remove(mask)
        held = V.pack(want.keys)
        mixed = RE.mixed_rows(keep)
        keys = RE.packed(mixed, RE.MANY_H)
        old, back = np.isin(keys, held), np.isin(keys, gone)
        assert len(mixed) == 3000 and old.sum() == 1400 and back.sum() == 10 * len(gone) and (~old & ~back).sum() >= 1500
        assert set(gone.tolist()) <= set(keys.tolist())
        # the insert does not grow the table: it goes into the one the removal refilled
        assert VI.table_log2(keep, 3000, after) == after and table.call(keep, 3000) == (1 << after, 0)
        grown = want.insert(mixed)
        assert grown == len(np.unique(keys[~old])) == len(gone) + (~old & ~back).sum() // 2
        # the leavers come back as new ids, among the new voxels in order of first appearance
        new_keys = V.pack(want.keys[keep:])
        first = np.unique(keys[~old], return_index=True)
        assert np.array_equal(new_keys, first[0][np.argsort(first[1])])
        at = np.flatnonzero(np.isin(new_keys, gone))
        assert len(at) == len(gone) and at.min() > 0 and at.max() < grown - 1


# ---- B ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", RE.RECORD_COUNTS)
def test_record_identity_case(m):
    assert [-(-c // E.CHUNK) for c in RE.RECORD_COUNTS] == [1, 1, 2, 3] and [c % E.CHUNK for c in RE.RECORD_COUNTS] == [2047, 0, 1, 1]
    rows, rec, again = RE.record_identity_case(m)
    assert len(rows) == (m + 1) // 2 and len(rec[0]) == len(again[0]) == m == len(set(V.pack(rec[0]).tolist()))
    assert not np.array_equal(rec[0], again[0]) and np.array_equal(np.sort(V.pack(rec[0])), np.sort(V.pack(again[0])))
    want = cloud_of(rows, RE.MANY_H)
    before = want.result()
    in_cloud = np.isin(V.pack(rec[0]), V.pack(want.keys))
    assert in_cloud.sum() == len(rows)
    grown = want.merge(*rec)
    assert grown == m - len(rows) == m // 2 and want.N == len(rows) + m
    assert want.subtract_records(*again) == grown
    same_cloud(want.result(), before)
    assert want.N == len(rows)
    # the table grows under the merge and shrinks again by the rule
    table = RE.Table(len(rows))
    built = table.now()[0]
    assert table.call(len(rows), m)[0] == 1 << VI.table_log2(len(rows), m, built.bit_length() - 1) > built
    assert table.kept(m, len(rows))[0] == 1 << VR.table_shrink_log2(len(rows), table.log2cap)


def test_records_past_one_pass_as_a_subtraction():
    head, h, rec = IE.records_case()
    M, grown, merged, N = IE.records_want()
    again = RE.records_again()
    m = len(rec[0])
    assert m > E.PASS and -(-m // E.CHUNK) == 299 > 256
    assert not np.array_equal(again[0], rec[0]) and np.array_equal(np.sort(V.pack(again[0])), np.sort(V.pack(rec[0])))
    assert int(again[1].sum()) == N - len(head) and (int(again[1].sum()) & 0xFFFFFFFF) == int(again[1].sum())
    # subtracting them all gives back the head's cloud: vectorised, as voxelremove._sub does it after its record check
    want = VR.Cloud(h)
    want.keys, want.n, want.S, want.SI, want.N = (merged["keys"].astype(np.int64), merged["counts"].astype(np.int64), merged["S"].copy(),
                                                  merged["SI"].copy(), N)
    assert want._sub(again[0].astype(np.int64), again[1], again[2], again[3], np.zeros(m, np.bool_)) == grown
    same_cloud(want.result(), V.downsample(head, h))
    assert want.N == len(head)
    # the refused record of the second pass, the lower of two
    keys, n, S, SI = IE.refused_records()
    bad = np.zeros(m, np.bool_)
    for i in (IE.RECORDS_BAD, IE.RECORDS_BAD + 1000):
        assert not VI.record_ok(keys[i], n[i], S[i], SI[i])
        bad[i] = True
    assert E.PASS < IE.RECORDS_BAD
    merged_cloud = VR.Cloud(h)
    merged_cloud.keys, merged_cloud.n, merged_cloud.S, merged_cloud.SI, merged_cloud.N = want_of(merged, N)
    K = keys.astype(np.int64)
    K[bad] = 0
    assert refusal(lambda: merged_cloud._sub(K, n, S, SI, bad))[:2] == (IE.RECORDS_BAD, VR.ITEM)
    # its key off the cloud instead, below a later record of count 0
    keys, n, S, SI = RE.records_missing()
    assert VI.record_ok(keys[IE.RECORDS_BAD], n[IE.RECORDS_BAD], S[IE.RECORDS_BAD], SI[IE.RECORDS_BAD])
    assert not np.isin(V.pack(keys[IE.RECORDS_BAD:IE.RECORDS_BAD + 1]), V.pack(merged["keys"])).any()
    bad = np.zeros(m, np.bool_)
    bad[IE.RECORDS_BAD + 1000] = True
    K = keys.astype(np.int64)
    K[bad] = 0
    assert refusal(lambda: merged_cloud._sub(K, n, S, SI, bad))[:2] == (IE.RECORDS_BAD, VR.MISSING)
    same_cloud(merged_cloud.result(), merged)


def want_of(d, N):
    return d["keys"].astype(np.int64), d["counts"].astype(np.int64), d["S"].copy(), d["SI"].copy(), N


def test_a_point_total_whose_low_word_is_zero():
    keys, n, S, SI = RE.POINTS_CASE
    assert all(VI.record_ok(keys[i], n[i], S[i], SI[i]) for i in range(4))
    total = int(n.sum())
    assert total == 4294967296 and total & 0xFFFFFFFF == 0 and str(total) in RE.POINTS_MESSAGE
    want = cloud_of(RE.POINTS_ROWS, RE.POINTS_H)
    assert want.N == 3 and want.keys.tolist() == [[0, 0, 0]]
    before = want.result()
    assert refusal(lambda: want.subtract_records(keys, n, S, SI)) == (-1, VR.POINTS, None)
    same_cloud(want.result(), before)


# ---- C ---------------------------------------------------------------------------------------------------------------
def wraps(keys, log2cap):
    """The keys held outnumber the slots from their lowest first slot to ``mask``: wherever each lands, the chain
    crosses to slot 0."""
    return len(keys) > (1 << log2cap) - int(E.slot_first(keys, log2cap).min())


def passes_a_hole(before, after, log2cap):
    """A survivor's first slot precedes the slot a removed key had in a table of this size (linear probing in id
    order; where the keys held before do not fit a table of this size, the removed key's first slot): the survivor's
    probe walks over the place the removed key left.  The keys form one chain that wraps, so "precedes" counts slots
    from the chain's start, the lowest first slot, round the table's end."""
    mask = (1 << log2cap) - 1
    removed = ~np.isin(before, after)
    if len(before) <= (1 << log2cap) // 2:
        _, steps = E.probe_model(before, log2cap)
        old = ((E.slot_first(before, log2cap) + steps) & mask)[removed]
    else:
        old = E.slot_first(before[removed], log2cap)
    start = int(E.slot_first(before, log2cap).min())
    return int(((E.slot_first(after, log2cap) - start) & mask).min()) < int(((old - start) & mask).max())


def check_plan(steps, done, kept, sizes):
    for k, ((kind, arg), (out, res, (slots, growths), before, after)) in enumerate(zip(steps, done)):
        log2cap = slots.bit_length() - 1
        assert len(res["keys"]) == len(after) == kept[k] and slots == sizes[k], (k, len(after), slots)
        assert len(after) <= slots // 2
        if len(after) > 0:
            assert wraps(after, log2cap), k                                  # the refilled chain crosses the table's end
        if kind != "insert" and len(after) > 0:
            assert out == len(before) - len(after) > 0 and passes_a_hole(before, after, log2cap), k
            assert np.array_equal(after, before[np.isin(before, after)])     # the survivors keep their order


def test_chain_plan_leaves_holes_inside_chains_that_wrap():
    k, held, a, b = RE.final_chain_rows()
    steps, done = RE.chain_plan()
    assert [kind for kind, _ in steps] == ["remove", "subtract", "insert", "remove", "remove", "remove", "insert"]
    start = V.downsample(held, IE.CHAIN_H)
    assert np.array_equal(V.pack(start["keys"]), V.pack(k)) and np.array_equal(done[0][3], V.pack(k))
    # the sizes by the two rules, step by step
    log2cap, sizes, kept = 15, [], [len(d[4]) for d in done]
    for (kind, arg), d in zip(steps, done):
        if kind == "insert":
            log2cap = VI.table_log2(len(d[3]), len(arg), log2cap)
        else:
            log2cap = VR.table_shrink_log2(len(d[4]), log2cap)
        sizes.append(1 << log2cap)
    assert kept[0] == 4111 >= (1 << 15) // 8 and sizes[0] == 1 << 15                   # no shrink: refilled in place
    assert VR.table_shrink_log2(6167 - 3084, 15) < 15                                  # which every second voxel would not give
    assert kept[1] < kept[0] and kept[2] == 6167 and kept[3:6] == [2000, 100, 3] and kept[6] == 6167
    assert sizes[3] == 1 << VR.table_shrink_log2(2000, sizes[2].bit_length() - 1) < sizes[2] and sizes[5] == 64
    assert [d[2][0] for d in done] == sizes and done[-1][2][1] > done[0][2][1] == 3
    check_plan(steps, done, kept, sizes)
    # step 2 empties voxels and leaves others with fewer points; step 3 meets survivors and brings the leavers back last
    assert 0 < done[1][0] < len(steps[1][1]) and done[1][1]["counts"].sum() == done[0][1]["counts"].sum() - len(steps[1][1])
    back = ~np.isin(done[2][4], done[2][3])
    assert done[2][0] == back.sum() > 2000 and not back[:kept[1]].any() and back[kept[1]:].all()
    assert np.array_equal(np.sort(done[2][4]), np.sort(V.pack(k)))
    # the last insert: three survivors met again, 6164 keys into 64 slots that grow
    assert done[6][0] == 6164 and sizes[6] == 1 << VI.table_log2(3, 6167, 6)
    # every key held is found by a subtraction of one of its points (the cloud holds at least one a or b row of each)
    final = done[-1][1]
    assert (final["counts"] >= 1).all()


def test_min_table_plan_keeps_the_64_slot_floor():
    steps, done, h = RE.min_table_plan()
    kept = [len(d[4]) for d in done]
    assert kept == [7, 1, 0, 65] and [kind for kind, _ in steps] == ["remove"] * 3 + ["insert"]
    log2cap, sizes = 8, []
    for keep in kept[:3]:
        log2cap = VR.table_shrink_log2(keep, log2cap)
        sizes.append(1 << log2cap)
    assert sizes == [64, 64, 64] and VI.LOG2_MIN == 6
    assert VR.table_shrink_log2(7, 8) == 6 and VR.table_shrink_log2(0, 6) == 6
    sizes.append(1 << VI.table_log2(0, 65, log2cap))
    assert [d[2][0] for d in done] == sizes and sizes[3] == 256 and [d[2][1] for d in done] == [3, 3, 3, 4]
    # seven survivors start in slots 62 and 63 and wrap; one survivor in its first slot cannot
    assert wraps(done[0][4], 6) and passes_a_hole(done[0][3], done[0][4], 6)
    assert (E.slot_first(done[0][4], 6) >= 62).all() and not wraps(done[1][4], 6)
    assert wraps(done[3][4], 8)
    _, parts, _ = IE.min_table_case()
    same_cloud(done[3][1], V.downsample(np.concatenate(parts), h))


# ---- D ---------------------------------------------------------------------------------------------------------------
def test_overdrawn_case():
    rows = RE.source()
    call, accepted, counts, counts_ok = RE.overdrawn_case()
    assert sum(counts) == len(call) == len(accepted) + RE.OVERDRAWN and sum(counts_ok) == len(accepted) and counts[1] == 0 == counts_ok[1]
    assert 5000 < len(call) <= len(rows) and len(counts) == 4
    want = cloud_of(rows, RE.SOURCE_H)
    before, M = want.result(), len(want.keys)
    held = dict(zip(V.pack(want.keys).tolist(), want.n.tolist()))
    keys = RE.packed(call, RE.SOURCE_H)
    uniq, taken = np.unique(keys, return_counts=True)
    left = np.array([held[key] for key in uniq.tolist()]) - taken
    assert (left == -1).sum() == RE.OVERDRAWN and (left == 0).sum() == RE.EMPTIED and (left == 1).sum() == len(uniq) - 90
    assert len(uniq) <= M and all(held[key] == 1 for key in set(held) - set(uniq.tolist()))      # a voxel of one point keeps it
    assert (taken[left == 1] >= 1).any() and taken[left == 1].sum() > 4000
    index, reason, key = refusal(lambda: want.subtract(call))
    over = uniq[left == -1]
    lowest = min(int(np.flatnonzero(keys == v)[0]) for v in over)
    assert reason == VR.REMAINDER and index == lowest < len(accepted) and V.pack(np.array([key]))[0] == keys[index]
    # the row that over-draws that voxel comes later, as do its other rows; and it is no point the cloud was given
    mine = np.flatnonzero(keys == keys[index])
    assert mine[0] == index and mine[-1] >= len(accepted) and len(mine) >= 2
    assert not (call[mine[-1]] == rows).all(axis=1).any()
    same_cloud(want.result(), before)
    assert want.N == 6000
    # as a batch: the frame and point of that row, behind an empty frame or not
    off = np.concatenate([[0], np.cumsum(counts)])
    f = int(np.searchsorted(off, index, side="right")) - 1
    assert counts[f] > 0 and 0 <= index - off[f] < counts[f]
    # without the extra points the call is accepted: the 40 and the 50 are emptied exactly
    assert want.subtract(accepted) == RE.OVERDRAWN + RE.EMPTIED and want.N == 6000 - len(accepted) == M - 90
    assert (want.n == 1).all()


def test_all_bad_and_far_apart_cases():
    rows = RE.source()
    want = cloud_of(rows, RE.SOURCE_H)
    before = want.result()
    nan, off = RE.all_bad_rows()
    assert len(nan) == len(off) == 5000 > 19 * RE.BLOCK
    assert V.quantise(nan[:, :3], nan[:, 3], RE.SOURCE_H, V.ZERO)[3].all()
    assert refusal(lambda: want.subtract(nan))[:2] == (0, VR.ITEM)
    found = np.isin(RE.packed(off, RE.SOURCE_H), V.pack(want.keys))
    assert found[0] and not found[1:].any()
    assert refusal(lambda: want.subtract(off))[:2] == (1, VR.MISSING)
    cases = RE.far_apart_cases()
    assert [(i, why) for _, i, why in cases] == [(3, VR.ITEM), (3, VR.MISSING)]
    for call, index, reason in cases:
        bad = V.quantise(call[:, :3], call[:, 3], RE.SOURCE_H, V.ZERO)[3]
        away = ~bad
        away[away] = ~np.isin(RE.packed(call[~bad], RE.SOURCE_H), V.pack(want.keys))
        assert bad.sum() == 1 == away.sum()
        lo, hi = sorted([int(np.flatnonzero(bad)[0]), int(np.flatnonzero(away)[0])])
        assert lo // RE.BLOCK == 0 and hi // RE.BLOCK == (len(call) - 1) // RE.BLOCK == 19 and lo == index
        assert refusal(lambda: want.subtract(call))[:2] == (index, reason)
    same_cloud(want.result(), before)


def test_refused_points_of_the_910_frames_as_a_subtraction():
    held, h = RE.frame_cloud()
    good, _ = E.frame_run_rows(False)
    counts = E.frame_run_counts()
    want = cloud_of(held, h)
    before = want.result()
    off = np.concatenate([[0], np.cumsum(counts)])
    cases = IE.refusal_cases()
    assert len(cases) == 9
    for what, at, (f, i, dense) in cases:
        assert dense == off[f] + i == min(at)
        assert refusal(lambda: want.subtract(IE.refused_rows(good, at)))[:2] == (dense, VR.ITEM), what
    same_cloud(want.result(), before)
    assert want.subtract(good) > 0
    same_cloud(want.result(), V.downsample(IE.other_points(), h))


# ---- E ---------------------------------------------------------------------------------------------------------------
def test_big_records_are_past_2_53():
    rows, h, o = E.big_sum_case()
    head, last, off = RE.big_records()
    assert (head[1] == E.BIG_N - 1).all() and len(head[0]) == 2
    whole = E.big_sum_want()
    assert (np.abs(head[2]) > 2 ** 53).any() and (whole["S"].astype(np.float64).astype(np.int64) != whole["S"]).any()      # a double loses bits
    assert all(VI.record_ok(head[0][i], head[1][i], head[2][i], head[3][i]) for i in range(2))
    want = VR.Cloud(h, o)
    want.keys, want.n, want.S, want.SI, want.N = want_of(whole, 2 * E.BIG_N)
    assert want.subtract_records(*head) == 0
    same_cloud(want.result(), last)
    assert want.N == 2 and (last["counts"] == 1).all()
    # the rows do the same (on a slice: the restatement of 4.4 million subtracted rows is the one of the records)
    sub = V.downsample(rows[:-2], h, o)
    assert np.array_equal(sub["S"], head[2]) and np.array_equal(sub["SI"], head[3]) and np.array_equal(sub["counts"], head[1])
    before = want.result()
    assert VI.record_ok(off[0][0], off[1][0], off[2][0], off[3][0])
    index, reason, key = refusal(lambda: want.subtract_records(*off))
    assert (index, reason, key) == (0, VR.REMAINDER, (0, 0, 0))
    same_cloud(want.result(), before)
    assert want.subtract(rows[-2:]) == 2 and want.N == 0 and len(want.keys) == 0


# ---- F ---------------------------------------------------------------------------------------------------------------
def test_layouts_as_subtracted_sources():
    other = IE.other_points()
    (c0, a0, b0), (c1, a1, b1) = IE.frame_halves()
    for one_voxel in (False, True):
        rows, h = E.frame_run_rows(one_voxel)
        want = cloud_of(other, h)
        want.insert(rows[a0:b0])
        want.insert(rows[a1:b1])
        gone = want.subtract(rows[a0:b0])
        assert gone == 0 if one_voxel else gone >= 0
        fresh = V.downsample(np.concatenate([other, rows[a1:b1]]), h)
        res = want.result()
        same_cloud(res, fresh, (by_key(res), by_key(fresh)))
        want.subtract(rows[a1:b1])
        same_cloud(want.result(), V.downsample(other, h))
    h, o = IE.WIDE_GRID
    for ld in (6, 7):
        rows = IE.wide_rows(ld)
        four = np.ascontiguousarray(rows[:, :4])
        want = cloud_of(four, h, o)
        M = len(want.keys)
        gone = want.subtract(rows[:IE.WIDE_CUT])
        assert 0 < gone < M and (want.n < V.downsample(four, h, o)["counts"][np.isin(V.pack(V.downsample(four, h, o)["keys"]), V.pack(want.keys))]).any()
        res, fresh = want.result(), V.downsample(four[IE.WIDE_CUT:], h, o)
        same_cloud(res, fresh, (by_key(res), by_key(fresh)))
    rows, times, h = IE.timed_case()
    want = cloud_of(rows, h)
    a = sum(IE.TIMED_COUNTS[0])
    assert 0 < want.subtract(rows[:a]) < len(V.downsample(rows, h)["keys"])
    res, fresh = want.result(), V.downsample(rows[a:], h)
    same_cloud(res, fresh, (by_key(res), by_key(fresh)))
    assert want.subtract(rows[a:]) == len(fresh["keys"]) and want.N == 0


def test_fuzz_parts_in_reverse_empty_the_cloud():
    for seed in E.FUZZ_SEEDS:
        h, o, rows64, rows32 = E.fuzz_case(seed)
        for cuts in (IE.FUZZ_ROW_CUTS, (0, 1000, 4096)):
            parts = IE.fuzz_parts(rows32, cuts)
            want = cloud_of(rows32, h, o)
            for k in range(len(parts) - 1, -1, -1):
                M = len(want.keys)
                gone = want.subtract(parts[k])
                # a part takes voxels out whole and leaves others with fewer points, but for the last, which empties
                assert (0 < gone < M) if k else gone == M, (seed, k)
                left = np.concatenate(parts[:k]) if k else np.zeros((0, 4))
                res, fresh = want.result(), V.downsample(left, h, o)
                if k:
                    same_cloud(res, fresh)      # the rows left are a prefix: the ids coincide with a fresh build's
            assert len(want.keys) == 0 == want.N
            want.insert(parts[0])
            same_cloud(want.result(), V.downsample(parts[0], h, o))


# ---- G ---------------------------------------------------------------------------------------------------------------
def final_keys(steps):
    return steps[-1][2]["keys"]


def test_window_case_grows_and_shrinks():
    frames, h = RE.window_case()
    steps = RE.window_want()
    assert len(frames) == RE.WINDOW_FRAMES == len(steps) == 40 and all(len(f) == RE.WINDOW_FRAME for f in frames)
    assert sum(RE.WINDOW_COUNTS) == RE.WINDOW_FRAME and 0 in RE.WINDOW_COUNTS
    checked = [i for i, s in enumerate(steps) if s[2] is not None]
    assert checked == [4, 9, 14, 19, 24, 29, 34, 39]
    for i, (grown, gone, res, at, N) in enumerate(steps):
        assert grown > 0 and (gone is None) == (i < RE.WINDOW) and (gone is None or gone > 0), i
        assert N == RE.WINDOW_FRAME * min(i + 1, RE.WINDOW)
    # every subtraction leaves voxels with fewer points as well as emptying some: the window's frames share voxels
    for i in range(RE.WINDOW, 40):
        assert steps[i][1] < len(V.downsample(frames[i - RE.WINDOW], h)["keys"]), i
    slots = [s[3][0] for s in steps]
    # the table grows with the window and then stays: 2667 voxels are more than an eighth of it
    assert max(slots) > slots[0] and slots[-1] == max(slots) and len(final_keys(steps)) >= slots[-1] // 8, slots
    final, fresh = steps[-1][2], V.downsample(np.concatenate(frames[35:]), h)
    same_cloud(final, fresh, (by_key(final), by_key(fresh)))
    assert len(fresh["keys"]) == 2667 and steps[-1][4] == 10000
    assert {RE.WINDOW_KINDS[i % 3] for i in range(RE.WINDOW, 40)} == set(RE.WINDOW_KINDS)


# ---- H ---------------------------------------------------------------------------------------------------------------
def test_moved_centroid_case():
    rows = R.corner_rows()
    take, far = RE.moved_centroid_case()
    want = cloud_of(rows, R.H)
    before = want.result()
    assert want.subtract(take) == 0
    after = want.result()
    assert np.array_equal(after["keys"], before["keys"]) and (after["counts"] >= 1).all()
    assert 100 < len(take) < len(before["keys"]) / 5 and after["counts"][far] == 1
    moved = np.abs(after["rows"][:, :3] - before["rows"][:, :3]).max(axis=1)
    assert moved[far] > R.H / 10 and (moved > 0).sum() > 100 and (moved == 0).sum() > 500
    left = rows[~(rows[:, None, :] == take[None, :, :]).all(axis=2).any(axis=1)]
    assert len(left) == len(rows) - len(take)
    fresh = V.downsample(left, R.H)
    same_cloud(after, fresh, (by_key(after), by_key(fresh)))
