"""The edge cases of a growing voxel cloud without a GPU: every builder of tests/voxelinsertedges.py holds the condition
that makes its case bite (tests/test_gpu_voxel_insert_edges.py runs the same cases on the kernels), checked on the NumPy
restatements of tests/voxel.py, voxelinsert.py and registration.py alone."""
import numpy as np
import pytest

import registration as R
import voxel as V
import voxeledges as E
import voxelinsert as VI
import voxelinsertedges as IE


def packed(rows, h, origin=V.ZERO):
    K, _, _, bad = V.quantise(rows[:, :3], rows[:, 3], h, origin)
    assert not bad.any()
    return V.pack(K)


def same_cloud(a, b):
    """Two restatement results (or V.downsample's dicts), every field to the bit."""
    for f in ("rows", "counts", "keys", "f32", "S", "SI"):
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f


# ---- A ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", E.SCAN_SIZES)
def test_grown_scan_case_carries_into_a_base_rank(size):
    head, call, counts, h = IE.grown_scan_case(size)
    M, grown, want = IE.grown_scan_want(size)
    n = len(call)
    assert len(head) == IE.HEAD and n == min(size, E.SCAN_SIZES[2] - IE.HEAD)
    assert counts.sum() == n and len(counts) == 11 and (counts == 0).sum() == 1 and (counts[counts > 0] % 256 != 0).all()
    chunks = -(-n // E.CHUNK)
    passes = -(-chunks // 256)
    assert (chunks, passes) == {E.SCAN_SIZES[0]: (256, 1), E.SCAN_SIZES[1]: (257, 2), E.SCAN_SIZES[2]: (513, 3)}[size]
    old = np.isin(packed(call, h), packed(head, h))
    first = np.zeros(n, bool)
    first[np.unique(packed(call, h), return_index=True)[1]] = True
    new_at = np.flatnonzero(first & ~old)           # the items k_vox_flag<true> flags
    assert M >= 900 and len(new_at) == grown == len(want["rows"]) - M
    assert new_at[-1] == n - 1 and want["counts"][-1] == 1                # the last item is new, a voxel of its own
    points = np.bincount(np.arange(n) // E.PASS, minlength=passes)
    per_pass = np.bincount(new_at // E.PASS, minlength=passes)
    met_again = np.bincount(np.flatnonzero(old) // E.PASS, minlength=passes)
    print(f"size {size}: M {M}, new per pass {per_pass.tolist()}, old voxels met per pass {met_again.tolist()}")
    # the builder opens a voxel every 5 to 13 items and picks one of the head's 1000 centres once in 200 items
    assert (per_pass >= np.minimum(100, points // 20)).all() and (met_again >= np.minimum(100, points // 500)).all()
    assert per_pass.min() >= 1 and (met_again[points > 1] >= 1).all()
    assert (new_at // E.CHUNK == chunks - 1).any()                        # the last chunk holds a first appearance
    per_chunk = np.bincount(new_at // E.CHUNK, minlength=chunks)
    assert all(len(set(per_chunk[p * 256:(p + 1) * 256].tolist())) > 1 for p in range(passes) if points[p] > E.CHUNK)
    # the grown cloud is the filter of head || call
    same_cloud(want, V.downsample(np.concatenate([head, call]), h))


def test_records_case_is_more_than_one_pass_of_repeated_keys():
    head, h, (keys, n, S, SI) = IE.records_case()
    M, grown, want, N = IE.records_want()
    m = len(keys)
    assert m == 610308 > E.PASS and -(-m // E.CHUNK) == 299 and len(head) == IE.RECORDS_HEAD
    uniq, times = np.unique(V.pack(keys), return_counts=True)
    assert len(uniq) == m // 6 and (times == 6).all()
    in_cloud = np.isin(uniq, packed(head, h))
    assert in_cloud.sum() > 1000 and grown == (~in_cloud).sum() > 1000
    # the accepted counts sum to what n_points reports, and the cloud is the filter of all the points six times over
    assert N == len(head) + int(n.sum()) == len(head) + 6 * (E.PASS + 1 - len(head))
    _, rows, _ = E.scan_case(E.PASS + 1)
    once = V.downsample(rows, h)
    assert np.array_equal(np.sort(V.pack(want["keys"])), np.sort(V.pack(once["keys"]))) and len(want["rows"]) == M + grown
    assert np.array_equal(want["keys"][:M], once["keys"][:M]) and not np.array_equal(want["keys"], once["keys"])
    # a record of the second pass refused: named by its own index, the lowest
    assert E.PASS < IE.RECORDS_BAD < m - 1000
    bad = IE.refused_records()
    assert not VI.record_ok(bad[0][IE.RECORDS_BAD], bad[1][IE.RECORDS_BAD], bad[2][IE.RECORDS_BAD], bad[3][IE.RECORDS_BAD])
    with pytest.raises(V.Refused) as e:
        VI.Cloud(h).merge(*bad)
    assert e.value.index == IE.RECORDS_BAD


# ---- B ---------------------------------------------------------------------------------------------------------------
def wraps(keys, log2cap):
    """The keys held outnumber the slots from their lowest first slot to ``mask``: wherever each lands, the chain
    crosses to slot 0."""
    return len(keys) > (1 << log2cap) - int(E.slot_first(keys, log2cap).min())


def test_live_chain_case_collides_in_every_table():
    k, steps = IE.live_chain_case()
    keys = V.pack(k)
    assert len(k) == 6167 == len(set(keys.tolist()))
    for log2cap in (12, 13, 14, 15):
        assert (E.slot_first(keys, log2cap) >= (1 << log2cap) - (96 << (log2cap - 12))).all()
    assert [kind for kind, _, _ in steps] == ["build", "rows", "rows", "batch", "rows", "records", "rows"]
    assert [len(rows) for _, rows, _ in steps] == [2048, 1, 4094, 4096, 1, 2103, 2093]
    assert [None if c is None else sum(c) for _, _, c in steps] == [None, None, None, 4096, None, None, None]
    done = IE.replay(steps, IE.CHAIN_H)
    assert tuple(at for _, _, at, _ in done) == IE.LIVE_CHAIN_TABLES
    assert [g for g, _, _, _ in done] == [2048, 1, 2047, 0, 1, 2003, 67]
    M = 0
    for (grown, res, (slots, _), items), (kind, rows, _) in zip(done, steps):
        held = V.pack(res["keys"])
        assert np.array_equal(held, keys[:len(held)])                  # the keys in the builder's order
        assert wraps(held, slots.bit_length() - 1) and len(held) <= slots // 2
        assert M == 0 or wraps(held[:M], slots.bit_length() - 1)       # what a growth rehashes wraps on its own
        M = len(held)
    # step 3: every new key twice, and 2049 old voxels in the way; step 4: exactly half load, nothing new, counts + 1
    assert np.array_equal(np.sort(done[2][3]), np.sort(np.repeat(keys[2049:4096], 2)))
    assert 4096 + 4096 == IE.LIVE_CHAIN_TABLES[3][0] // 2 and set(done[3][3].tolist()) == set(keys[:4096].tolist())
    assert np.array_equal(done[3][1]["counts"][:4096], done[2][1]["counts"] + 1)
    # step 6: records of new keys, then of the cloud's first 100; step 7 rehashes 6100 keys
    assert np.isin(done[5][3][:2003], keys[:4097]).sum() == 0 and np.array_equal(done[5][3][2003:], keys[:100])
    # the final cloud's centroids are their own nearest voxels at distance 0
    final = done[-1][1]
    assert len(final["rows"]) == 6167
    ids, d2 = R.nearest(final["keys"], final["rows"][:, :3], IE.CHAIN_H, V.ZERO, final["rows"][:, :3], IE.CHAIN_H / 2)
    assert np.array_equal(ids, np.arange(6167)) and (d2 == 0.0).all()


def test_min_table_case_collides_from_64_slots_on():
    k, steps, h = IE.min_table_case()
    keys = V.pack(k)
    assert len(set(keys.tolist())) == 65 and E.chain_keys(7, 124, 1, 0)[1] == 8213
    assert (E.slot_first(keys, 6) >= 60).all() and (E.slot_first(keys, 7) >= 124).all() and (E.slot_first(keys, 8) >= 248).all()
    done = IE.replay(steps, h)
    assert tuple(at for _, _, at, _ in done) == IE.MIN_TABLES and [g for g, _, _, _ in done] == [32, 1, 31, 1]
    assert IE.Table().now() == (0, 0)
    for _, res, (slots, _), _ in done:
        held = V.pack(res["keys"])
        assert wraps(held, slots.bit_length() - 1) and len(held) <= slots // 2
    assert len(done[2][1]["keys"]) == 64 == done[2][2][0] // 2          # exactly half load of 128 slots


# ---- C ---------------------------------------------------------------------------------------------------------------
def test_frame_halves_and_refusal_cases():
    counts = E.frame_run_counts()
    halves = IE.frame_halves()
    assert [len(c) for c, _, _ in halves] == [455, 455] and halves[0][2] == halves[1][1] and halves[1][2] == counts.sum()
    (c0, a0, b0), (c1, a1, b1) = halves
    assert c0.sum() == b0 - a0 and c1.sum() == b1 - a1
    assert c0[:2].tolist() == [0, 0] and c0[-3:].tolist() == [0, 0, 1] and c1[:2].tolist() == [0, 0] and c1[-3:].tolist() == [0, 0, 0]
    assert all({255, 256, 257, 513} <= set(c.tolist()) for c in (c0, c1))
    other = IE.other_points()
    for one_voxel in (False, True):
        rows, h = E.frame_run_rows(one_voxel)
        assert not (rows[:, None, :3] == other[None, :7, :3]).all(axis=2).any()
        # in two calls from nothing, and in one call into the other points' cloud: the filter of the concatenation
        want = VI.Cloud(h)
        g0, g1 = want.insert(rows[a0:b0]), want.insert(rows[a1:b1])
        assert (g0, g1) == ((1, 0) if one_voxel else (1728, 0))          # the second half meets the first half's voxels only
        same_cloud(want.result(), V.downsample(rows, h))
        want = VI.Cloud(h)
        M = want.insert(other)
        grown = want.insert(rows)
        assert M > 100 and (grown == 0 if one_voxel else 0 < grown < len(V.downsample(rows, h)["rows"]))
        same_cloud(want.result(), V.downsample(np.concatenate([other, rows]), h))
    cases = IE.refusal_cases()
    assert len(cases) == 9 and [len(at) for _, at, _ in cases] == [1] * 6 + [2] * 3
    rows, h = E.frame_run_rows(False)
    off = np.concatenate([[0], np.cumsum(counts)])
    for what, at, (f, i, dense) in cases:
        assert dense == min(at) == off[f] + i and 0 <= i < counts[f], what
        cloud = VI.Cloud(h)
        cloud.insert(other)
        with pytest.raises(V.Refused) as e:
            cloud.insert(IE.refused_rows(rows, at))
        assert e.value.index == dense and cloud.N == 3000, what
    lowest = {c[2][2] for c in cases}
    assert {0, int(counts.sum()) - 1} <= {d for _, at, _ in cases for d in at} and 0 in lowest and len(lowest) == 6


# ---- D ---------------------------------------------------------------------------------------------------------------
def test_fuzz_parts_meet_old_keys_and_new_ones():
    assert sum(sum(c) for c in IE.FUZZ_BATCHES) == 4096 and sum(IE.FUZZ_BATCHES, ()) == E.FUZZ_COUNTS
    for seed in E.FUZZ_SEEDS:
        h, o, rows64, rows32 = E.fuzz_case(seed)
        for rows, cuts in ((rows32, (0, 1000, 4096)), (rows64, IE.FUZZ_ROW_CUTS)):
            want, seen = VI.Cloud(h, o), np.zeros(0, np.int64)
            for k, part in enumerate(IE.fuzz_parts(rows, cuts)):
                keys = packed(part, h, o)
                old = np.isin(keys, seen)
                assert k == 0 or (old.any() and not old.all()), (seed, k)
                want.insert(part)
                seen = np.union1d(seen, keys)
            same_cloud(want.result(), V.downsample(rows, h, o))
        # the records of the first part into the cloud of the second
        first, second = rows64[:2049], rows64[2049:]
        want = VI.Cloud(h, o)
        want.insert(second)
        grown = want.merge(*VI.records_of(V.downsample(first, h, o)))
        assert 0 < grown < len(V.downsample(first, h, o)["rows"])
        same_cloud(want.result(), V.downsample(np.concatenate([second, first]), h, o))


# ---- E ---------------------------------------------------------------------------------------------------------------
def test_layout_cases():
    h, o = IE.WIDE_GRID
    for ld in (6, 7):
        rows = IE.wide_rows(ld)
        assert rows.shape == (3001, ld) and np.isfinite(rows[:, :4]).all()
        assert (~np.isfinite(rows[:, 4:]) | (rows[:, 4:] == 1e308)).all() and (~np.isfinite(rows[:, 4:])).any(axis=1).mean() > 0.8
        old = np.isin(packed(rows[IE.WIDE_CUT:], h, o), packed(rows[:IE.WIDE_CUT], h, o))
        assert old.any() and not old.all()
        # a junk column read as a coordinate or an intensity is refused, or lands elsewhere
        for c in range(4, ld):
            shifted = np.array(rows[:, :4])
            shifted[:, 3] = rows[:, c]
            with pytest.raises(V.Refused):
                V.downsample(shifted, h, o)
    rows, times, h = IE.timed_case()
    assert len(rows) == len(times) == 2257 and times.min() < -2 ** 30 and times.max() > 2 ** 30
    assert np.array_equal(rows, E.f32(rows))
    (a, _), (b, c) = IE.TIMED_COUNTS
    old = np.isin(packed(rows[a:], h), packed(rows[:a], h))
    assert old.any() and not old.all() and b % 256 == 1


# ---- F ---------------------------------------------------------------------------------------------------------------
def test_corner_parts_share_voxels_and_bring_new_ones():
    parts = IE.corner_parts()
    rows = R.corner_rows()
    assert [len(p) for p in parts] == [400, 600, len(rows) - 1000]
    whole = V.downsample(rows, R.H)
    want, seen = VI.Cloud(R.H), np.zeros(0, np.int64)
    for k, part in enumerate(parts):
        d = V.downsample(part, R.H)
        old = np.isin(V.pack(d["keys"]), seen)
        assert k == 0 or (old.any() and not old.all())
        want.merge(*VI.records_of(d))
        seen = np.union1d(seen, V.pack(d["keys"]))
    same_cloud(want.result(), whole)
    M = len(whole["rows"])
    mask = IE.corner_mask(M)
    assert mask.dtype == np.bool_ and mask.shape == (M,) and 200 < mask.sum() < M
    assert len(IE.corner_mask(len(V.downsample(np.concatenate(parts[:2]), R.H)["rows"]))) < M      # the old mask is shorter
    # the extra point: a voxel of its own, next to the cloud
    p = IE.corner_extra_point()
    k = V.quantise(p[:, :3], p[:, 3], R.H, V.ZERO)[0]
    assert not np.isin(V.pack(k), V.pack(whole["keys"])).any()
    assert np.isin(V.pack(k - [0, 0, 1]), V.pack(whole["keys"])).all()
