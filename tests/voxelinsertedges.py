"""Shared builders of the edge tests of a growing voxel cloud (tests/test_voxel_insert_edges_cpu.py,
tests/test_gpu_voxel_insert_edges.py): numpy only, deterministic seeds, on top of the one-shot filter's builders in
tests/voxeledges.py.

Each builder aims at one place where the insert path of csrc/voxel.hpp / voxel.hip (k_vox_validate, k_vox_rehash,
k_vox_insert_live, k_vox_flag<true>, k_vox_scan, k_vox_rank<true>, k_vox_accumulate_items, grow_table, the host insert)
can go wrong without tests/test_gpu_voxel_insert.py noticing, and states in its docstring the condition that makes its
case bite; test_voxel_insert_edges_cpu.py asserts that condition on the restatements (tests/voxel.py, voxelinsert.py)
alone, and the GPU tests compare with the restatements only.

  grown_scan_case   one insert of more than one pass of k_vox_scan into a cloud that has voxels: the carry between
                    passes meets a base rank M > 0
  records_case      more than one pass of records, keys repeated: k_vox_validate<records> over 299 workgroups
  live_chain_case   keys that collide in every table size, through builds, growths, re-observations and a merge
  min_table_case    the same from an empty cloud through the 64-, 128- and 256-slot tables
  frame_halves, refusal_cases, other_points
                    the 910-frame batch of voxeledges as an insert source, and the naming of refused points in it
  fuzz_parts        the fuzz grids cut into calls
  wide_rows, timed_case
                    rows of 6 and 7 columns and a batch with a time column as insert sources
  corner_parts, corner_mask, corner_extra_point
                    the corner cloud of tests/registration.py in three parts, for the analyses of a grown cloud
"""
import functools

import numpy as np

import registration as R
import voxel as V
import voxeledges as E
import voxelinsert as VI


class Table:
    """(slots, growths) as mc_voxel_table reports them, by the growth rule of include/mcdeskew.h restated in
    voxelinsert.table_log2: ``built`` the points of the one-shot build (0: an empty source, no table yet)."""

    def __init__(self, built=0):
        self.log2cap = E.table_log2(built) if built else 0
        self.growths = 0

    def call(self, M, n):
        """An accepted call of n items on a cloud of M voxels."""
        if n:
            log2cap = VI.table_log2(M, n, self.log2cap)
            self.growths += log2cap != self.log2cap
            self.log2cap = log2cap
        return self.now()

    def now(self):
        return ((1 << self.log2cap) if self.log2cap else 0, self.growths)


def point_records(rows, h, origin=V.ZERO):
    """Every point as a record of its own (keys, n = 1, S, SI): what a merge takes."""
    K, Q, QI, bad = V.quantise(rows[:, :3], rows[:, 3], h, origin)
    assert not bad.any()
    return K.astype(np.int32), np.ones(len(K), np.int64), Q, QI


# ---- A: more than one scan pass in one call, on a cloud that has voxels ----------------------------------------------
HEAD = 5000


@functools.lru_cache(maxsize=None)
def grown_scan_case(size):
    """-> (head (HEAD, 4), call, counts of the call as a batch, h): rows[:HEAD] of the largest scan case build the
    cloud, rows[HEAD:HEAD + size] are one insert (the largest size ends with the source, 5000 rows short: still three
    passes), the last item moved into a voxel nobody else has.  Bites when, relative to the head's cloud, the call has
    first appearances in every pass of 256 x 2048 items and in its last chunk, its last item is new, and the head's
    M > 0 voxels are met again in every pass: k_vox_rank<true> adds M to ranks that carry k_vox_scan's carry."""
    _, rows, h = E.scan_case(E.SCAN_SIZES[2])
    call = np.array(rows[HEAD:HEAD + size])
    call[-1, :3] = E.f32((np.array([-200.0, 200.0, -200.0]) + 0.5) * h)
    return E.frozen(np.array(rows[:HEAD])), E.frozen(call), E.frozen(E.uneven_counts(len(call))), h


@functools.lru_cache(maxsize=None)
def grown_scan_want(size):
    """-> (M of the head's cloud, new voxels of the call, the restatement's result)"""
    head, call, _, h = grown_scan_case(size)
    want = VI.Cloud(h)
    M = want.insert(head)
    grown = want.insert(call)
    return M, grown, want.result()


RECORDS_HEAD = 100000
RECORDS_BAD = E.PASS + 4321           # a record of the second pass


@functools.lru_cache(maxsize=None)
def records_case():
    """-> (head rows, h, (keys, n, S, SI)): the cloud of rows[:100 000] of the 524 289-row scan case, and the records
    of the voxel filter of the rest six times over, each copy in another seeded order.  Bites when the records are
    more than one pass of 256 x 2048 (k_vox_scan's carry, k_vox_validate's one 64-bit add per 2048 records from 299
    workgroups), every key occurs six times, and some keys are the cloud's and some are new."""
    _, rows, h = E.scan_case(E.PASS + 1)
    d = V.downsample(rows[RECORDS_HEAD:], h)
    rng = np.random.default_rng(6)
    order = np.concatenate([rng.permutation(len(d["keys"])) for _ in range(6)])
    rec = tuple(E.frozen(np.ascontiguousarray(a[order])) for a in VI.records_of(d))
    return E.frozen(np.array(rows[:RECORDS_HEAD])), h, rec


@functools.lru_cache(maxsize=None)
def records_want():
    """-> (M of the head's cloud, new voxels of the merge, the restatement's result, N afterwards)"""
    head, h, rec = records_case()
    want = VI.Cloud(h)
    M = want.insert(head)
    grown = want.merge(*rec)
    return M, grown, want.result(), want.N


def refused_records():
    """records_case's records with record RECORDS_BAD, and a later one, of count 0."""
    keys, n, S, SI = records_case()[2]
    n = np.array(n)
    n[[RECORDS_BAD, RECORDS_BAD + 1000]] = 0
    return keys, n, S, SI


# ---- B: probe chains in a live, growing table ------------------------------------------------------------------------
CHAIN_H = 0.5


def chain_rows(k, h, seed):
    """One dyadic point in every voxel of k, as voxeledges.probe_case builds them."""
    rng = np.random.default_rng(seed)
    rows = np.column_stack([(k + rng.integers(1, 8, (len(k), 3)) / 8.0) * h, rng.integers(0, 256, len(k)) / 256.0])
    assert np.array_equal(rows, E.f32(rows))
    return rows


@functools.lru_cache(maxsize=None)
def live_chain_case():
    """-> (k (6167, 3), steps): every cube key whose first slot is in the last 96 of 4096 slots, in a seeded order, and
    the calls (kind, rows, frame counts or None), the first a one-shot build; records are one per row.  The hash takes
    the key's top bits, so the same keys start in the last 2^-12 * 96 of every larger table.  Bites when at every step
    the keys held outnumber the slots from their lowest first slot to ``mask`` (the chain wraps to slot 0 whatever the
    arrival order), k_vox_rehash places keys that all collide again, and new keys walk over old voxels' slots.

    The table after each call is what the growth rule gives (LIVE_CHAIN_TABLES).  An insert counts its items, not its
    new keys (M + items > slots / 2 grows): the one item of step 2 rehashes 2048 colliding keys into 8192 slots, the
    4094 items of step 3 (2047 new keys, each twice) rehash 2049 into 16 384 before the new keys walk over them, step 4
    meets every voxel again at exactly half load (4096 + 4096 = 16 384 / 2) without growing, steps 5 and 6 add a key and
    merge records through the same chains, and step 7 (the 67 keys left and 2026 keys met again) crosses half load once
    more and rehashes 6100 colliding keys at once."""
    k, total = E.chain_keys(12, 4000, 1 << 18, 21)
    assert total == len(k)
    a, b = chain_rows(k, CHAIN_H, 22), chain_rows(k, CHAIN_H, 23)
    again = 2049 + np.random.default_rng(24).permutation(2047)
    steps = (("build", a[:2048], None),
             ("rows", a[2048:2049], None),
             ("rows", np.concatenate([a[2049:4096], b[again]]), None),
             ("batch", a[:4096], (1024, 0, 3072)),
             ("rows", a[4096:4097], None),
             ("records", np.concatenate([a[4097:6100], a[:100]]), None),
             ("rows", np.concatenate([a[6100:], b[:2026]]), None))
    return E.frozen(k), tuple((kind, E.frozen(rows), counts) for kind, rows, counts in steps)


LIVE_CHAIN_TABLES = ((4096, 0), (8192, 1), (16384, 2), (16384, 2), (16384, 2), (16384, 2), (32768, 3))


@functools.lru_cache(maxsize=None)
def min_table_case():
    """-> (k (65, 3), steps, h): keys whose first slot is >= 124 of 128 (hence >= 62 of 64 and >= 248 of 256), inserted
    into an empty cloud as 32, 1, 31 and 1 rows: the 64-slot minimum table made by the first insert, grown to 128, filled
    to exactly half load without growing, grown to 256.  Bites as live_chain_case does."""
    k, _ = E.chain_keys(7, 124, 65, 25)
    rows = chain_rows(k, 1.0, 26)
    return E.frozen(k), tuple(E.frozen(rows[a:b]) for a, b in ((0, 32), (32, 33), (33, 64), (64, 65))), 1.0


MIN_TABLES = ((64, 1), (128, 2), (128, 2), (256, 3))


def replay(steps, h, origin=V.ZERO):
    """The restatement through the steps of live_chain_case / min_table_case -> per step (new voxels, result(), table,
    packed keys of the step's items)."""
    want, table, out = VI.Cloud(h, origin), None, []
    for step in steps:
        kind, rows = step[:2] if isinstance(step, tuple) else ("rows", step)
        M = len(want.keys)
        if kind == "build":
            table = Table(len(rows))
        elif table is None:
            table = Table()
        grown = want.merge(*point_records(rows, h, origin)) if kind == "records" else want.insert(rows)
        at = table.now() if kind == "build" else table.call(M, len(rows))
        out.append((grown, want.result(), at, V.pack(V.quantise(rows[:, :3], rows[:, 3], h, origin)[0])))
    return out


# ---- C: runs of empty frames as an insert source, refusal naming -----------------------------------------------------
def frame_halves():
    """-> [(counts, first row, end row)] of frames 0..454 and 455..909 of voxeledges.frame_run_counts: the first batch
    ends with the one-point frame behind two empty frames, the second begins with two and ends with three empty
    frames.  Bites when both halves hold points, empty frames at both ends and frames of 255, 256, 257 and 513."""
    counts = E.frame_run_counts()
    off = np.concatenate([[0], np.cumsum(counts)])
    return [(counts[:455], int(off[0]), int(off[455])), (counts[455:], int(off[455]), int(off[910]))]


@functools.lru_cache(maxsize=None)
def other_points():
    """3000 points that are none of frame_run_rows', in the same cube: the cloud an insert of the 910 frames grows."""
    rng = np.random.default_rng(42)
    return E.frozen(E.f32(np.column_stack([rng.uniform(-3.0, 3.0, (3000, 3)), rng.uniform(0.0, 1.0, 3000)])))


def refusal_cases():
    """-> [(what, {dense index: refused row}, (frame, point, dense index) of the lowest)]: every place of
    voxeledges.refusal_places with its row of REFUSED_ROWS, and the three two-at-once combinations of
    test_gpu_voxel_edges.test_refusals_are_named_among_empty_frames.  Bites when the lowest refused point is the
    first or last of the batch next to empty frames, the one-point frame, or at points 255, 256, 512 of a frame."""
    places = E.refusal_places()
    cases = [(name, {p[2]: E.REFUSED_ROWS[k]}) for k, (name, p) in enumerate(places.items())]
    first, last, lone, p255, p256, p512 = (p[2] for p in places.values())
    cases += [("two at once", {p256: E.REFUSED_ROWS[0], last: E.REFUSED_ROWS[1]}),
              ("two at once, the lower in the one-point frame", {lone: E.REFUSED_ROWS[3], p512: E.REFUSED_ROWS[2]}),
              ("the first and the last point", {first: E.REFUSED_ROWS[4], last: E.REFUSED_ROWS[5]})]
    by_dense = {p[2]: p for p in places.values()}
    return [(what, at, by_dense[min(at)]) for what, at in cases]


def refused_rows(good, at):
    rows = np.array(good)
    for dense, row in at.items():
        rows[dense] = row
    return rows


# ---- D: grids --------------------------------------------------------------------------------------------------------
FUZZ_BATCHES = ((1000, 0), (2000, 1096))     # voxeledges.FUZZ_COUNTS as two batches
FUZZ_ROW_CUTS = (0, 1, 2049, 4096)


def fuzz_parts(rows, cuts):
    """Bites when a later part holds keys the earlier parts brought and keys that are new."""
    return [rows[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- E: layouts ------------------------------------------------------------------------------------------------------
WIDE_GRID = (0.3, (0.1, 0.2, 0.3))
WIDE_CUT = 1000
JUNK = (np.nan, np.inf, -np.inf, 1e308)


@functools.lru_cache(maxsize=None)
def wide_rows(ld):
    """3001 rows of ld columns: x, y, z, intensity, then columns of NaN, +-inf and 1e308 that no kernel may read as
    a coordinate.  Bites when every row holds a non-finite extra value and the cut leaves old and new keys."""
    rng = np.random.default_rng(ld)
    rows = np.empty((3001, ld))
    rows[:, :4] = rng.uniform(-4, 4, (3001, 4))
    rows[:, 4:] = rng.choice(JUNK, (3001, ld - 4))
    return E.frozen(rows)


TIMED_COUNTS = ((700, 0), (257, 1300))


@functools.lru_cache(maxsize=None)
def timed_case():
    """-> (rows holding float32 values, int32 times, h): a batch with a time column is five columns per block, so
    a source read with the four-column stride lands in the times, which as float32 bits are anything."""
    rng = np.random.default_rng(70)
    n = sum(sum(c) for c in TIMED_COUNTS)
    return E.frozen(E.f32(rng.uniform(-4, 4, (n, 4)))), E.frozen(rng.integers(-2 ** 31, 2 ** 31, n)), 0.3


# ---- F: what a grown cloud invalidates -------------------------------------------------------------------------------
CORNER_CUTS = (0, 400, 1000)


def corner_parts():
    """The corner cloud's rows in the three parts of test_the_analyses_see_the_grown_cloud.  Bites when every later
    part holds voxels of the earlier ones and new ones: a merge of their states adds into records and appends."""
    rows = R.corner_rows()
    cuts = CORNER_CUTS + (len(rows),)
    return [rows[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def corner_mask(M):
    """Two voxels of three, by id."""
    return np.arange(M) % 3 != 1


def corner_extra_point(h=R.H):
    """One point in a voxel of its own right above the z patch's first cell: its neighbours' normals, the cluster it
    joins and that cluster's bounding box all change."""
    return np.array([[1.0 + h / 2, 1.0 + h / 2, 1.5 * h, 0.5]])
