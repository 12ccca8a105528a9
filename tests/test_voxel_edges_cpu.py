"""The voxel filter's edge cases without a GPU: every builder of tests/voxeledges.py holds the condition
that makes its case bite (tests/test_gpu_voxel_edges.py runs the same cases on the kernels), checked on
the NumPy restatement of tests/voxel.py alone."""
import numpy as np
import pytest

import voxel as V
import voxeledges as E


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- A -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.SCAN_SIZES)
def test_scan_case_has_first_appearances_in_every_pass(n):
    counts, rows, h = E.scan_case(n)
    assert len(rows) == n and counts.sum() == n and len(counts) == 11
    assert (counts == 0).sum() == 1 and counts[0] > 0 and counts[-1] > 0
    assert (counts[counts > 0] % 256 != 0).all() and len(set(counts.tolist())) == 11
    first = E.first_appearances(rows, h)
    want = E.scan_want(n)
    assert len(first) == len(want["rows"]) and first[-1] == n - 1 and want["counts"][-1] == 1   # the last point's own voxel
    chunks = -(-n // E.CHUNK)
    passes = -(-chunks // 256)
    assert (chunks, passes) == {E.SCAN_SIZES[0]: (256, 1), E.SCAN_SIZES[1]: (257, 2), E.SCAN_SIZES[2]: (516, 3)}[n]
    per_pass = np.bincount(first // E.PASS, minlength=passes)
    points = np.bincount(np.arange(n) // E.PASS, minlength=passes)
    print(f"n {n}: {len(first)} voxels, first appearances per pass {per_pass.tolist()}")
    # every pass holds at least 100 first appearances (the one-point pass of 256 * 2048 + 1: its point)
    assert (per_pass >= np.minimum(100, points)).all()
    if n == E.SCAN_SIZES[2]:
        assert (per_pass >= 100).all() and n % E.CHUNK == 17 and chunks % 256 == 4
    # and chunks of every pass differ in their counts: an offset taken from the wrong chunk shows
    per_chunk = np.bincount(first // E.CHUNK, minlength=chunks)
    assert all(len(set(per_chunk[p * 256:(p + 1) * 256].tolist())) > 1 for p in range(passes) if points[p] > E.CHUNK)


# ---- B -------------------------------------------------------------------------------------------------------
def test_slot_first_is_the_fibonacci_hash():
    """Against Python integers; and the count of cube keys that start in the last 96 of 4096 slots."""
    C, W = 0x9E3779B97F4A7C15, 1 << 64
    k = E.cube_keys()
    keys = V.pack(k)
    assert len(set(keys.tolist())) == 64 ** 3
    for log2cap in (6, 12):
        want = [((key * C) % W) >> (64 - log2cap) for key in keys[::97].tolist()]
        assert E.slot_first(keys[::97], log2cap).tolist() == want
    assert E.chain_keys(12, 4000, 1, 0)[1] == 6167
    assert E.chain_keys(6, 60, 1, 0)[1] >= 32


@pytest.mark.parametrize("which", range(len(E.PROBE_CASES)))
def test_probe_case_wraps_and_goes_far(which):
    counts, rows, h, k = E.probe_case(which)
    n = len(rows)
    assert sum(counts) == n == (2048, 2048, 32)[which]
    log2cap = E.table_log2(n)
    assert log2cap == (12, 12, 6)[which]
    mask = (1 << log2cap) - 1
    K, _, _, bad = V.quantise(rows[:, :3], rows[:, 3], h, (0, 0, 0))
    assert not bad.any() and np.array_equal(K, k)
    keys = V.pack(K)
    n_keys = len(set(keys.tolist()))
    assert n_keys == (2048, 512, 32)[which]
    assert (E.slot_first(keys, log2cap) >= (4000, 4000, 60)[which]).all()
    occupied, steps = E.probe_model(keys, log2cap)
    print(f"{E.PROBE_CASES[which]}: longest probe {steps.max()} of {n_keys} keys, {len(occupied)} slots taken")
    assert len(occupied) == n_keys and mask in occupied and 0 in occupied
    # the chain crosses from slot mask to slot 0 and is at least half the keys long (a chain cannot be
    # longer than the keys there are, so with four points per key the keys are the measure)
    assert steps.max() >= n_keys // 2
    if which == 0:
        assert steps.max() >= 2000
    if which == 1:      # every key comes back in both frames, and walks its chain again
        first_frame = set(keys[:1024].tolist())
        assert len(first_frame) == 512 and set(keys[1024:].tolist()) == first_frame
        assert steps[1536:].max() >= n_keys // 2
    want = V.downsample(rows, h)
    assert len(want["rows"]) == n_keys and (want["counts"] == n // n_keys).all()


# ---- C -------------------------------------------------------------------------------------------------------
def test_big_sums_are_inexact_in_float64_and_their_last_bit_shows():
    rows, h, o = E.big_sum_case()
    want = E.big_sum_want()
    n = E.BIG_N
    assert n > 2 ** 21 and want["keys"].tolist() == [[0, 0, 0], [1, 1, 0]] and want["counts"].tolist() == [n, n]
    S, SI = want["S"], want["SI"]
    q = 2 ** 32 - 1
    assert S[0].tolist() == [n * q, n * (q - 2), n * 2 ** 31] and S[1].tolist() == [n * q, n * 2 ** 30, n * 3 * 2 ** 30]
    assert SI.tolist() == [n * q, -n * q]
    assert int(S[0, 0]) == 9448932343967295 and S[0, 0] > 2 ** 53 and S[0, 0] % 4 == 3     # rounds up, away from truncation
    assert S[0, 1] > 2 ** 53 and S[0, 1] % 4 == 1                                           # rounds down
    assert float(S[0, 0]) == float(int(S[0, 0]) + 1) and float(S[0, 1]) == float(int(S[0, 1]) - 1)
    assert abs(int(SI[0])) > 2 ** 53 and SI[0] % 2 == 1
    # a sum off by one, or converted by truncation, changes output bits
    base = V.finalise(want["keys"], S, SI, want["counts"], h, o)
    assert np.array_equal(bits(base), bits(want["rows"]))
    differs = []
    for d in (-1, 1):
        other = V.finalise(want["keys"], S + d, SI + d, want["counts"], h, o)
        differs.append(bits(other) != bits(base))
        print(f"S {d:+d}: x of voxel 0 {float(other[0, 0]).hex()} against {float(base[0, 0]).hex()}")
    assert (differs[0] | differs[1])[0, 0] and (differs[0] | differs[1])[0, 1] and (differs[0] | differs[1])[0, 3]
    trunc = V.finalise(want["keys"], S & ~1, SI & ~1, want["counts"], h, o)
    assert bits(trunc)[0, 0] != bits(base)[0, 0]


# ---- D -------------------------------------------------------------------------------------------------------
def test_frame_runs_and_refusal_places():
    counts = E.frame_run_counts()
    assert 890 <= len(counts) <= 910
    assert counts[:3].tolist() == [0, 0, 0] and counts[-3:].tolist() == [0, 0, 0] and counts[-4] == 257
    one = np.flatnonzero(counts == 1)
    lone = [f for f in one if not counts[f - 2:f].any() and not counts[f + 1:f + 3].any()]
    off = np.concatenate([[0], np.cumsum(counts)])
    places = E.refusal_places()
    assert len(places) == 6 and len({p[2] for p in places.values()}) == 6
    for name, (f, i, dense) in places.items():
        assert 0 <= i < counts[f] and dense == off[f] + i, name
    assert places["first point of the first non-empty frame"][2] == 0
    assert places["last point of the last non-empty frame"][2] == counts.sum() - 1
    assert [places["one-point frame between empty frames"][0]] == lone
    assert all(counts[places[f"point {i} of a 513-point frame"][0]] == 513 for i in (255, 256, 512))
    for one_voxel in (True, False):
        rows, h = E.frame_run_rows(one_voxel)
        assert len(rows) == counts.sum()
        want = V.downsample(rows, h)
        assert (len(want["rows"]) == 1) if one_voxel else (len(want["rows"]) > 1000)
        for k, (name, (f, i, dense)) in enumerate(places.items()):
            bad = np.array(rows)
            bad[dense] = E.REFUSED_ROWS[k]
            with pytest.raises(V.Refused) as e:
                V.downsample(bad, h)
            assert e.value.index == dense, name
    for row in E.REFUSED_ROWS:
        assert np.array_equal(np.asarray(row), E.f32(row), equal_nan=True)     # a batch can hold them


# ---- E -------------------------------------------------------------------------------------------------------
def test_fuzz_grids_refuse_nothing_and_fill_voxels():
    hs, scales = [], set()
    for seed in E.FUZZ_SEEDS:
        h, o, rows64, rows32 = E.fuzz_case(seed)
        assert 1e-3 <= h <= 1e2 and rows64.shape == (4096, 4) and sum(E.FUZZ_COUNTS) == 4096
        hs.append(h)
        scales.add(seed % 3)
        for rows in (rows64, rows32):
            want = V.downsample(rows, h, o)          # raises Refused on any refused point
            shared = (want["counts"] >= 2).mean()
            assert shared >= 0.25, (seed, h, o, shared)
        assert not np.array_equal(rows64, rows32)
    assert len(E.FUZZ_SEEDS) == 24 and scales == {0, 1, 2}
    assert min(hs) < 1e-2 and max(hs) > 10 and len(set(hs)) == 24


# ---- F -------------------------------------------------------------------------------------------------------
def test_own_voxel_sizes_cover_the_lane_tails_and_the_small_tables():
    assert {n % 4 for n in E.OWN_SIZES} == {0, 1, 2, 3}
    assert {E.table_log2(n) for n in E.OWN_SIZES} >= {6, 7}
    assert E.table_log2(32) == 6 and E.table_log2(33) == 7 and E.table_log2(2048) == 12 and E.table_log2(2049) == 13
    for n in E.OWN_SIZES + (2049,):
        rows, keys = E.own_voxel_rows(n)
        want = V.downsample(rows, 0.25)
        assert len(want["rows"]) == n and np.array_equal(want["keys"], keys)
    rows, keys = E.own_voxel_rows(2049, 0.125, (16.0, -8.0, 4.0))
    assert np.array_equal(V.downsample(rows, 0.125, (16.0, -8.0, 4.0))["keys"], keys)
