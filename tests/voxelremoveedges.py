"""Shared builders of the edge tests of a shrinking voxel cloud (tests/test_voxel_remove_edges_cpu.py,
tests/test_gpu_voxel_remove_edges.py): numpy only, deterministic seeds, on top of the builders of tests/voxeledges.py,
voxelinsertedges.py and registration.py.

Each builder aims at one place where the way out of csrc/voxel.hpp / voxel.hip (k_vox_keep, k_vox_compact, k_vox_refill,
k_vox_sub_validate, k_vox_sub_apply, k_vox_sub_check, vox_block_add, vox_lowest, the hosts' compact, keep_voxels,
keep_flags and subtract) can go wrong without tests/test_gpu_voxel_remove.py noticing, and states in its docstring the
condition that makes its case bite; test_voxel_remove_edges_cpu.py asserts that condition on the restatements
(tests/voxel.py, voxelinsert.py, voxelremove.py) alone, and the GPU tests compare with the restatements only.

  many_voxels, masks, shrink_edge, mixed_rows
                    A  more than 256 workgroups of voxels under a removal, the shrink rule's edge at that size, and a
                       mixed insert into the table a removal refilled in place
  record_identity_case, records_again, records_missing, POINTS_CASE
                    B  records past one workgroup of k_vox_sub_validate<records> and past one pass, and a point total
                       whose low word is not the total
  chain_plan, min_table_plan
                    C  the colliding keys of voxelinsertedges under removals: holes inside chains that wrap
  overdrawn_case, all_bad_rows, far_apart_cases, frame_cloud
                    D  refusals that undo thousands of items
  big_records       E  the two voxels of voxeledges.big_sum_case as records past 2^53
  window_case       G  a sliding window of five frames over forty
  moved_centroid_case
                    H  a subtraction that empties no voxel and moves a centroid
"""
import functools

import numpy as np

import registration as R
import voxel as V
import voxeledges as E
import voxelinsertedges as IE
import voxelremove as VR

BLOCK = 256                      # kVoxBlock: voxels per workgroup of k_vox_keep, k_vox_compact and k_vox_refill
SCAN_PASS = 256                  # workgroups one pass of the selection scan in compact() takes


class Table(IE.Table):
    """voxelinsertedges.Table with the way down: (slots, growths) after a call that left M_keep of M voxels, by the
    shrink rule of include/mcdeskew.h restated in voxelremove.table_shrink_log2.  A shrink is no growth."""

    def kept(self, M, M_keep):
        if M_keep != M:
            self.log2cap = VR.table_shrink_log2(M_keep, self.log2cap)
        return self.now()


def packed(rows, h, origin=V.ZERO):
    K, _, _, bad = V.quantise(rows[:, :3], rows[:, 3], h, origin)
    assert not bad.any()
    return V.pack(K)


# ---- A: past 256 workgroups of voxels --------------------------------------------------------------------------------
MANY = (65536, 65537, 131329)    # 256, 257 and 514 workgroups of 256 voxels (513 and one voxel)
MANY_H = 0.25


def own_keys(i):
    """The voxel index of own voxel i, as test_gpu_voxel_remove.own_voxels numbers them."""
    i = np.asarray(i, np.int64)
    return np.stack([i % 13 - 6, (i // 13) % 17 - 8, i // 221 - 4], axis=1)


def own_rows(i, seed):
    """One dyadic point in own voxel i[j] for every j (exact in float32 and in the filter's fixed point)."""
    rng = np.random.default_rng(seed)
    rows = np.column_stack([(own_keys(i) + rng.integers(1, 8, (len(i), 3)) / 8.0) * MANY_H, rng.integers(0, 256, len(i)) / 256.0])
    assert np.array_equal(rows, E.f32(rows))
    return rows


@functools.lru_cache(maxsize=None)
def many_voxels(M):
    """-> rows (2 M, 4): M distinct voxels of two points each, voxel v's points at rows 2 v and 2 v + 1, so voxel ids
    are the voxel numbers.  Bites when M is more than 256 workgroups of 256 voxels (the selection scan of compact()
    takes a second pass, k_vox_compact's vox_block_add sums the points of more than 256 workgroups into one word) and
    M is no multiple of 256 for the two larger sizes (a tail workgroup)."""
    return E.frozen(own_rows(np.repeat(np.arange(M), 2), M))


def masks(M):
    """name -> (M,) bool of the voxels that leave.  Bites when a mask cuts inside the first pass, at its last voxel
    (65 535), at the first voxel of the second pass (65 536), at the cloud's ends, everywhere (alternate, a tenth) and
    nowhere but one voxel (the complement of a single voxel leaves one survivor, M' = 1)."""
    v = np.arange(M)
    out = {"alternate": v % 2 == 0, "only voxel 0": v == 0, "only the last voxel": v == M - 1,
           "only voxel 65535": v == 65535, "everything from 65536 on": v >= 65536,
           "a seeded tenth": np.random.default_rng(M).random(M) < 0.1, "all but voxel 40000": v != 40000}
    if M > 65536:
        out["only voxel 65536"] = v == 65536
    return out


MASK_NAMES = ("alternate", "only voxel 0", "only the last voxel", "only voxel 65535", "only voxel 65536",
              "everything from 65536 on", "a seeded tenth", "all but voxel 40000")
MANY_CASES = tuple((M, name) for M in MANY for name in MASK_NAMES if M > 65536 or name != "only voxel 65536")
EDGE_M = MANY[1]


def shrink_edge():
    """-> (slots of the one-shot build of many_voxels(65 537), the survivors that keep that table, one fewer).  The
    rule: fewer than slots / 8 survivors shrink the table.  The figures come from voxeledges.table_log2."""
    slots = 1 << E.table_log2(2 * EDGE_M)
    return slots, slots // 8, slots // 8 - 1


def edge_mask(keep):
    """The voxels of the 65 537 that leave so that ``keep`` stay: spread over both scan passes."""
    gone = EDGE_M - keep
    mask = np.zeros(EDGE_M, np.bool_)
    mask[[1000, 65536 - 7][:gone] if gone <= 2 else np.arange(gone)] = True
    assert mask.sum() == gone
    return mask


@functools.lru_cache(maxsize=None)
def mixed_rows(keep):
    """3000 rows to insert after edge_mask(keep): in a seeded order 1400 rows of survivors' keys (700 voxels, twice
    each), 10 rows of every voxel that has just left, and the rest in some 790 voxels nobody had, twice each.  Bites when
    the table the insert goes into is the one k_vox_refill filled (in place for the first ``keep``, newly allocated
    for the second) and does not grow, so the leavers' keys must find empty slots whose first index is "none", the
    survivors' keys slots whose first index is below 2^31, and the leavers come back as new ids in order of first
    appearance among the new voxels."""
    gone = np.flatnonzero(edge_mask(keep))
    rng = np.random.default_rng(keep)
    stay = rng.choice(np.flatnonzero(~edge_mask(keep)), 700, replace=False)
    new = EDGE_M + 5 + np.arange((3000 - 1400 - 10 * len(gone)) // 2)
    i = np.concatenate([np.repeat(stay, 2), np.repeat(gone, 10), np.repeat(new, 2)])
    extra = 3000 - len(i)
    i = np.concatenate([i, new[:extra]])
    return E.frozen(own_rows(i[rng.permutation(3000)], keep + 1))


# ---- B: records past one workgroup and one scan pass -----------------------------------------------------------------
RECORD_COUNTS = (2047, 2048, 2049, 4097)      # a workgroup of k_vox_sub_validate<records> takes kVoxChunk = 2048


@functools.lru_cache(maxsize=None)
def record_identity_case(m):
    """-> (rows of the cloud, records to merge (keys, n, S, SI), the same records in another order): the cloud holds
    one point in every second of m own voxels, the records are one per voxel, each a point of its own.  Bites when m
    is just below, at, just above one workgroup of 2048 records and past two (a tail in a later round of the kPer
    loop, a second workgroup of one record), half of the keys are the cloud's, and the two orders differ."""
    cloud = own_rows(np.arange(0, m, 2), m)
    rng = np.random.default_rng(m)
    rec = IE.point_records(own_rows(np.arange(m), m + 1), MANY_H)
    a, b = rng.permutation(m), rng.permutation(m)
    return E.frozen(cloud), tuple(E.frozen(np.ascontiguousarray(x[a])) for x in rec), \
        tuple(E.frozen(np.ascontiguousarray(x[b])) for x in rec)


@functools.lru_cache(maxsize=None)
def records_again():
    """voxelinsertedges.records_case's 610 308 records in one more seeded order: what a subtraction takes back out of
    the merged cloud.  Bites when the records are more than one pass of 256 x 2048 and 299 workgroups add into
    meta[2..3], and the order is neither the merge's nor sorted."""
    rec = IE.records_case()[2]
    order = np.random.default_rng(66).permutation(len(rec[0]))
    assert not np.array_equal(order, np.arange(len(order)))
    return tuple(E.frozen(np.ascontiguousarray(a[order])) for a in rec)


RECORDS_OFF = 4000               # added to a key: off the cube the scan case's centres lie in


def records_missing():
    """records_case's records with record RECORDS_BAD moved to a voxel the cloud lacks and the record 1000 later of
    count 0: two kinds of refusal in the second pass, the lower one MISSING."""
    keys, n, S, SI = IE.records_case()[2]
    keys, n = np.array(keys), np.array(n)
    keys[IE.RECORDS_BAD] += RECORDS_OFF
    n[IE.RECORDS_BAD + 1000] = 0
    return keys, n, S, SI


# a cloud of three points in voxel (0, 0, 0), and four records of that key with n = 2^30 and sums of 0: every record
# passes record_ok, together they bring 2^32 points, and the low word of that total is 0
POINTS_H = 1.0
POINTS_ROWS = E.frozen(np.array([[0.25, 0.25, 0.25, 0.5], [0.5, 0.5, 0.5, 0.25], [0.75, 0.75, 0.75, 0.0]]))
POINTS_CASE = (np.zeros((4, 3), np.int32), np.full(4, 1 << 30, np.int64), np.zeros((4, 3), np.int64), np.zeros(4, np.int64))
POINTS_MESSAGE = r"brings 4294967296 points and the cloud holds 3"


# ---- C: holes inside chains ------------------------------------------------------------------------------------------
def final_chain_rows():
    """-> (k, every row the final cloud of live_chain_case holds, a, b): the sources of its seven steps."""
    k, steps = IE.live_chain_case()
    return k, np.concatenate([rows for _, rows, _ in steps]), IE.chain_rows(k, IE.CHAIN_H, 22), IE.chain_rows(k, IE.CHAIN_H, 23)


@functools.lru_cache(maxsize=None)
def chain_plan():
    """-> (steps, done): the calls on the final cloud of voxelinsertedges.live_chain_case (6167 keys that start in the
    last 96 of every 4096 slots, in 32 768 slots), as (kind, argument) with kind "remove" (a mask over the cloud as
    it is then), "subtract" or "insert" (rows), and per step what the restatement gives: (the call's result, result(),
    (slots, growths), packed keys held before, packed keys held after).

    Bites when after every step the survivors outnumber the slots from their lowest first slot to ``mask`` (the
    refilled chain wraps) and a survivor's first slot precedes the slot a removed key had (its probe passes the hole):
    a lookup that stops at a hole, or a refill that leaves a key behind one, loses a voxel.  test_voxel_remove_edges_cpu
    asserts both with voxeledges.probe_model in the table after the step.

    Two figures differ from the round ones one would write down first, by the rule itself: every second voxel of 6167
    leaves 3083, fewer than an eighth of 32 768, which shrinks the table, so the first removal takes every third voxel
    (4111 stay, the table stays); and one survivor cannot outnumber the one slot it starts in, so the last removal keeps
    three (64 slots, first slots 62 and 63)."""
    k, held, a, b = final_chain_rows()
    want = VR.Cloud(IE.CHAIN_H)
    want.insert(held)
    table = Table()
    table.log2cap, table.growths = 15, 3
    assert table.now() == IE.LIVE_CHAIN_TABLES[-1]
    rng = np.random.default_rng(27)
    steps, done = [], []

    def run(kind, arg):
        before, M = V.pack(want.keys), len(want.keys)
        if kind == "remove":
            out = want.remove(arg)
            at = table.kept(M, M - out)
        elif kind == "subtract":
            out = want.subtract(arg)
            at = table.kept(M, M - out)
        else:
            out = want.insert(arg)
            at = table.call(M, len(arg))
        steps.append((kind, E.frozen(np.array(arg))))
        done.append((out, want.result(), at, before, V.pack(want.keys)))

    run("remove", np.arange(len(want.keys)) % 3 == 0)
    ids = np.flatnonzero(np.isin(V.pack(k), V.pack(want.keys)))           # the builder's numbers of the survivors
    third = ids[rng.random(len(ids)) < 1.0 / 3.0]
    run("subtract", a[third])                                              # empties the voxels that held a[i] alone
    run("insert", b)                                                       # survivors met again, leavers come back
    for keep in (2000, 100, 3):
        mask = np.ones(len(want.keys), np.bool_)
        mask[rng.choice(len(mask), keep, replace=False)] = False
        run("remove", mask)
    run("insert", a)
    return tuple(steps), tuple(done)


@functools.lru_cache(maxsize=None)
def min_table_plan():
    """As chain_plan on voxelinsertedges.min_table_case: from 65 keys in 256 slots down to 7, 1 and 0 voxels (the
    64-slot floor of the rule each time), then the 65 rows again."""
    k, parts, h = IE.min_table_case()
    rows = np.concatenate(parts)
    want = VR.Cloud(h)
    want.insert(rows)
    table = Table()
    table.log2cap, table.growths = 8, 3
    assert table.now() == IE.MIN_TABLES[-1]
    rng = np.random.default_rng(28)
    steps, done = [], []
    for keep in (7, 1, 0):
        M, before = len(want.keys), V.pack(want.keys)
        mask = np.ones(M, np.bool_)
        mask[rng.choice(M, keep, replace=False)] = False
        out = want.remove(mask)
        steps.append(("remove", E.frozen(mask)))
        done.append((out, want.result(), table.kept(M, keep), before, V.pack(want.keys)))
    before = V.pack(want.keys)
    out = want.insert(rows)
    steps.append(("insert", E.frozen(np.array(rows))))
    done.append((out, want.result(), table.call(0, len(rows)), before, V.pack(want.keys)))
    return tuple(steps), tuple(done), h


# ---- D: refusals that must undo much ---------------------------------------------------------------------------------
SOURCE_H = 0.2


@functools.lru_cache(maxsize=None)
def source():
    """The 6000 float32-exact points over 900 cells of test_gpu_voxel_remove.source()."""
    rng = np.random.default_rng(1)
    centre = rng.integers(-20, 20, (900, 3))
    pick = rng.integers(0, 900, 6000)
    return E.frozen(E.f32(np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (6000, 3))) * SOURCE_H, rng.uniform(-3, 3, 6000)])))


OVERDRAWN, EMPTIED = 40, 50
OVERDRAWN_COUNTS = (1500, 0, 2000)            # and a fourth frame of what is left


@functools.lru_cache(maxsize=None)
def overdrawn_case():
    """-> (call, accepted, frame counts of call, of accepted): ``call`` is one subtraction from the cloud of source()
    in which 40 voxels get every point they hold and one point more (their counts pass 0 and wrap), 50 other voxels
    get exactly the points they hold, and every other voxel all its points but one; ``accepted`` is the call without
    the 40 extra points, in the same order.  The rows are in a seeded order with the 40 extra points last.

    Bites when the call is thousands of items of which 40 voxels' worth are invalid (k_vox_sub_apply(+1) must bring
    back every count, the wrapped ones too, and every sum), other voxels stand at a count of 0 when the call is
    refused (nothing may compact), the lowest item of an invalid voxel is one of the cloud's own points and not the
    point that over-draws it, and several invalid voxels compete for the lowest item (vox_lowest).

    The call cannot be the 6000 rows one would write down first: a call that brings more points than the cloud holds
    is refused for that alone, before any voxel is looked at; it is 5237 rows (a voxel of one point keeps it and gives
    none).  And without the extra points the 40 voxels are emptied exactly like the 50: the accepted call empties 90."""
    rows = source()
    vox = packed(rows, SOURCE_H)
    uniq = np.unique(vox)
    rng = np.random.default_rng(31)
    pick = rng.permutation(len(uniq))
    over, gone = uniq[pick[:OVERDRAWN]], uniq[pick[OVERDRAWN:OVERDRAWN + EMPTIED]]
    take = np.ones(len(rows), np.bool_)
    rest = ~np.isin(vox, np.concatenate([over, gone]))
    last = {}
    for i in np.flatnonzero(rest):
        last[vox[i]] = i
    take[list(last.values())] = False                     # every other voxel keeps its last point
    accepted = rows[take][rng.permutation(int(take.sum()))]
    first = np.array([np.flatnonzero(vox == v)[0] for v in over])
    extra = np.array(rows[first])
    extra[:, 3] = 0.5                                     # one more point of each over-drawn voxel, not one it holds
    call = np.concatenate([accepted, extra[rng.permutation(OVERDRAWN)]])
    counts = lambda n: OVERDRAWN_COUNTS + (n - sum(OVERDRAWN_COUNTS),)
    return E.frozen(call), E.frozen(accepted), counts(len(call)), counts(len(accepted))


def all_bad_rows():
    """-> (5000 rows of NaN: every item refused, row 0 the lowest; 5000 rows of which row 0 is source()'s and all others
    lie 100 m off the cloud: row 1 the lowest MISSING).  Bites when every lane of 20 workgroups has an item for
    vox_lowest's one word."""
    off = np.array(source()[:5000])
    off[1:, 0] += 100.0
    return np.full((5000, 4), np.nan), off


def far_apart_cases():
    """-> [(rows, index, reason)]: source()'s first 5000 rows with a NaN in the first workgroup and a point off the
    cloud in the last, the NaN lower; and the reverse.  The lowest refused item decides the kind, whichever word of
    meta it is in."""
    lo, hi = 3, 5000 - 2
    out = []
    for bad, away, reason in ((lo, hi, VR.ITEM), (hi, lo, VR.MISSING)):
        rows = np.array(source()[:5000])
        rows[bad, 1] = np.nan
        rows[away, 0] += 100.0
        out.append((rows, lo, reason))
    return out


def frame_cloud():
    """-> (the rows of a cloud that holds other_points() and then the 910 frames, h)."""
    good, h = E.frame_run_rows(False)
    return np.concatenate([IE.other_points(), good]), h


# ---- E: sums past 2^53 -----------------------------------------------------------------------------------------------
def big_records():
    """-> (records of big_sum_case's rows[:-2] (two, n = 2 200 000 each), V.downsample of rows[-2:], the record of voxel
    (0, 0, 0)'s last point with SI off by one).  Bites when the sums subtracted are past 2^53 (a subtraction through
    a double loses the low bits) and what is left is one point's exact quantities."""
    rows, h, o = E.big_sum_case()
    whole, last = E.big_sum_want(), V.downsample(rows[-2:], h, o)
    assert np.array_equal(whole["keys"], last["keys"])
    head = (whole["keys"], whole["counts"].astype(np.int64) - 1, whole["S"] - last["S"], whole["SI"] - last["SI"])
    off = (last["keys"][:1], np.ones(1, np.int64), last["S"][:1], last["SI"][:1] + 1)
    return head, last, off


# ---- G: a sliding window ---------------------------------------------------------------------------------------------
WINDOW, WINDOW_FRAMES, WINDOW_FRAME = 5, 40, 2000
WINDOW_KINDS = ("rows", "batch", "state")
WINDOW_COUNTS = (700, 0, 1300)


def window_case():
    """-> (frames: 40 arrays of 2000 rows of voxeledges.scan_case(PASS + 1), h).  Step i inserts frame i and, from i = 5
    on, subtracts frame i - 5, the sources alternating rows, batch and state by i % 3.  Bites when every subtraction
    empties voxels and leaves others, every insert meets voxels of the window and brings new ones, and the table grows
    while the window fills and is then left alone by both rules."""
    _, rows, h = E.scan_case(E.PASS + 1)
    return [rows[f * WINDOW_FRAME:(f + 1) * WINDOW_FRAME] for f in range(WINDOW_FRAMES)], h


@functools.lru_cache(maxsize=None)
def window_want():
    """The restatement through window_case -> per step i (new voxels, emptied voxels or None, result() at every fifth
    step and at the last, (slots, growths), N)."""
    frames, h = window_case()
    want, table, out = VR.Cloud(h), Table(), []
    for i, rows in enumerate(frames):
        M = len(want.keys)
        items = len(V.downsample(rows, h)["keys"]) if WINDOW_KINDS[i % 3] == "state" else len(rows)
        grown = want.insert(rows)
        table.call(M, items)
        gone = None
        if i >= WINDOW:
            M = len(want.keys)
            gone = want.subtract(frames[i - WINDOW])
            table.kept(M, M - gone)
        out.append((grown, gone, want.result() if i % 5 == 4 or i == len(frames) - 1 else None, table.now(), want.N))
    return tuple(out)


# ---- H: what a shrunk cloud invalidates ------------------------------------------------------------------------------
def moved_centroid_case():
    """-> (rows of the corner cloud to subtract, the voxel id whose centroid moves): one of the two points of every
    sixth voxel of registration.corner_rows(), among them the voxel whose two points lie furthest apart.  No voxel
    empties, so no id changes; bites when that voxel's centroid moves by more than a tenth of a voxel, so normals,
    cluster statistics and a registration computed from centroids kept from before show."""
    rows = R.corner_rows()
    d = V.downsample(rows, R.H)
    vox = packed(rows, R.H)
    order = {key: v for v, key in enumerate(V.pack(d["keys"]).tolist())}
    vid = np.array([order[key] for key in vox.tolist()])
    spread = np.zeros(len(d["keys"]))
    firsts = {}
    for i, v in enumerate(vid.tolist()):
        if v in firsts:
            spread[v] = np.abs(rows[i, :3] - rows[firsts[v], :3]).max()
        else:
            firsts[v] = i
    far = int(np.argmax(spread))
    chosen = (np.arange(len(spread)) % 6 == far % 6)
    take = np.array([firsts[v] for v in np.flatnonzero(chosen).tolist()])
    return E.frozen(np.array(rows[np.sort(take)])), far
