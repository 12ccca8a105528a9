"""The kept normals of a voxel cloud without a GPU (include/mcdeskew.h "kept normals"): (1) the definition itself, in
the restatement of tests/keptnormals.py: stale rows patched on the dirty set D alone are the fresh estimate of the edited
cloud in every bit, over random sequences of edits, and D has no member to spare on constructed cases; (2) the marking
of csrc/normals_core.hpp (window walk, claim rule, epochs), included by tests/host/kept_normals_host.cpp, built with g++
plainly and under ASan + UBSan, against the restatement's D; (3) the module surface that needs no device."""
import os
import re
import shutil

import numpy as np
import pytest

import hostbuild
import keptnormals as K
import normals as N
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT
H = 0.25
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


# ---- (1) the definition ----------------------------------------------------------------------------------------------
def random_edits(cloud, rng):
    """A sequence of edits of every kind on `cloud`, each as (name, function of the cloud as it is then -> Edit)."""
    lo, hi = cloud.keys.min(axis=0), cloud.keys.max(axis=0) + 1
    fresh_cells = rng.integers(lo - 2, hi + 2, (12, 3))                    # mostly new voxels, at and beyond the rim
    frame = np.concatenate([K.cells_rows(fresh_cells, H, rng), K.cells_rows(cloud.keys[rng.integers(0, len(cloud), 15)], H, rng)])
    other = K.Cloud.of_rows(K.cells_rows(rng.integers(lo, hi, (10, 3)), H, rng), H)

    def take_whole(c):                                                     # a subtraction that empties voxels
        ids = rng.permutation(len(c))[:5]
        return K.subtract(c, c.records(ids))

    return [("insert", lambda c: K.add(c, K.items_of_rows(c, frame))),
            ("merge", lambda c: K.add(c, other.records(np.arange(len(other))))),
            ("unmerge", lambda c: K.subtract(c, other.records(np.arange(len(other))))),
            ("subtract", lambda c: K.subtract(c, K.items_of_rows(c, frame))),
            ("subtract that empties", take_whole),
            ("remove", lambda c: K.remove(c, rng.uniform(size=len(c)) < 0.02)),
            ("insert into one voxel", lambda c: K.add(c, K.items_of_rows(c, K.cells_rows(c.keys[[len(c) // 2] * 3], H, rng))))]


@pytest.mark.parametrize("rel,M", [(1.0, 3000), (2.0, 1500), (4.0, 500)])
@pytest.mark.parametrize("max_nn", [0, 3, 30])
def test_patching_the_dirty_set_alone_is_the_fresh_estimate(rel, M, max_nn):
    rng = np.random.default_rng(1000 * int(rel) + max_nn)
    cloud = K.Cloud.of_rows(K.sheet(M, seed=M + max_nn, h=H), H)
    assert len(cloud) == M
    radius, R = rel * H, int(rel)
    est = cloud.estimate(radius, max_nn)
    carried = 0
    for name, edit_of in random_edits(cloud, rng):
        e = edit_of(cloud)
        D = K.dirty(e, R)
        fresh = e.after.estimate(radius, max_nn)
        assert K.same(K.patch(est, fresh, e, D), fresh), (name, rel, max_nn)
        assert 0 < len(D) < len(e.after), name
        carried += len(e.after) - len(D)
        cloud, est = e.after, fresh
    assert carried > 0


def star(rng=None):
    """A voxel and its six face neighbours, every point moved a tenth of a cell towards the middle, so that at radius h
    (R = 1) the middle voxel is a neighbour of each and each of the middle, and two far voxels nothing is near to."""
    cells = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [40, 0, 0], [0, -40, 7]])
    rows = K.cells_rows(cells, H)
    rows[1:7, :3] -= 0.1 * H * cells[1:7]
    return cells, rows


BITE_CASES = ("insert into a voxel", "insert a new voxel", "merge", "subtract", "subtract that empties", "remove")


@pytest.mark.parametrize("kind", BITE_CASES)
def test_the_dirty_set_has_no_member_to_spare(kind):
    """On the star, every member of D is a voxel whose row the edit really changes: patching on D without it fails."""
    cells, rows = star()
    moved = rows[:1] + [0.05 * H, -0.03 * H, 0.02 * H, 0.0]                 # a second point of the middle voxel
    if kind == "insert into a voxel":
        cloud = K.Cloud.of_rows(rows, H)
        e = K.add(cloud, K.items_of_rows(cloud, moved))
    elif kind == "insert a new voxel":
        cloud = K.Cloud.of_rows(rows[1:], H)
        e = K.add(cloud, K.items_of_rows(cloud, rows[:1]))
    elif kind == "merge":
        cloud = K.Cloud.of_rows(rows, H)
        e = K.add(cloud, K.Cloud.of_rows(moved, H).records([0]))
    elif kind == "subtract":
        cloud = K.Cloud.of_rows(np.concatenate([rows, moved]), H)
        e = K.subtract(cloud, K.items_of_rows(cloud, moved))
    elif kind == "subtract that empties":
        cloud = K.Cloud.of_rows(rows, H)
        e = K.subtract(cloud, K.items_of_rows(cloud, rows[:1]))
    else:
        cloud = K.Cloud.of_rows(rows, H)
        e = K.remove(cloud, np.arange(len(cloud)) == 0)
    stale, fresh = cloud.estimate(H, 30), e.after.estimate(H, 30)
    D = K.dirty(e, 1)
    gone = kind in ("subtract that empties", "remove")
    assert len(D) == (6 if gone else 7) and len(e.after) == len(D) + 2
    assert K.same(K.patch(stale, fresh, e, D), fresh)
    for d in D:
        assert not K.same(K.patch(stale, fresh, e, D[D != d]), fresh), (kind, int(d))


# ---- (2) the core under g++ --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kept_normals_host")
    return tmp, [hostbuild.build(tmp, "kept_normals_host.cpp", sanitize=san) for san in (False, True)]


def mark(exe, tmp, keys, R, edits, epoch=0, n_points=None):
    """The harness on a cloud of these keys, its table sized as the build sizes it (>= 2 N slots, 64 at least):
    -> per edit (epoch, cleared, claimed, listed ids)."""
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
    log2cap = 6
    while (1 << log2cap) < 2 * (n_points or len(keys)):
        log2cap += 1
    blob = np.array([len(keys), R, log2cap, epoch, len(edits)], np.int64).tobytes() + keys.tobytes()
    for items in edits:
        items = np.ascontiguousarray(items, np.uint32)
        blob += np.array([len(items)], np.int64).tobytes() + items.tobytes()
    src, dst = tmp / "in.bin", tmp / "out.bin"
    src.write_bytes(blob)
    hostbuild.run(exe, src, dst)
    raw, out, at = dst.read_bytes(), [], 0
    for _ in edits:
        head = np.frombuffer(raw, np.int64, 4, at)
        ids = np.frombuffer(raw, np.uint32, int(head[3]), at + 32)
        out.append((int(head[0]), int(head[1]), int(head[2]), ids.astype(np.int64)))
        at += 32 + 4 * int(head[3])
    assert at == len(raw)
    return out


def ids_of(cloud, cells):
    at = {int(p): i for i, p in enumerate(V.pack(cloud.keys))}
    return np.array([at[int(p)] for p in V.pack(cells)], np.int64)


@needs_gxx
@pytest.mark.parametrize("R", [1, 2, 4])
def test_core_marks_the_restatement_s_dirty_set(exes, R):
    tmp, builds = exes
    rng = np.random.default_rng(R)
    cloud = K.Cloud.of_rows(K.sheet(2000, seed=R, h=H), H)
    frame = np.concatenate([K.cells_rows(rng.integers(-12, 12, (5, 3)), H, rng), K.cells_rows(cloud.keys[rng.integers(0, 2000, 12)], H, rng)])
    grown = K.add(cloud, K.items_of_rows(cloud, frame))
    K_items = K.items_of_rows(cloud, frame)[0]
    gone = K.remove(cloud, rng.uniform(size=2000) < 0.005)
    for exe in builds:
        # an insert: the items' voxels in the grown cloud, a voxel as often as items land in it
        (_, _, claimed, got), = mark(exe, tmp, grown.after.keys, R, [ids_of(grown.after, K_items)])
        D = K.dirty(grown, R)
        assert claimed == len(grown.touched) and len(got) == len(set(got.tolist())) and np.array_equal(np.sort(got), D)
        assert 0 < len(D) < len(grown.after)
        # a removal: the removed voxels mark on the old ids; the survivors among the marked, under their new ids, are D
        removed = np.setdiff1d(np.arange(2000), gone.carry)
        (_, _, _, got), = mark(exe, tmp, cloud.keys, R, [removed])
        new_id = np.full(2000, -1)
        new_id[gone.carry] = np.arange(len(gone.after))
        assert np.array_equal(np.sort(new_id[np.setdiff1d(got, removed)]), K.dirty(gone, R))


@needs_gxx
def test_core_at_both_ends_of_the_key_range(exes):
    """The cells of N.key_ends(): windows that reach over the range's ends, and decoys where a key packed without the
    range check would land."""
    tmp, builds = exes
    rows, h = N.key_ends()[:2]
    cloud = K.Cloud.of_rows(rows, h)
    for R in (1, 2, 4):
        for v in range(len(cloud)):
            e = K.add(cloud, K.items_of_rows(cloud, rows[v:v + 1]))
            for exe in builds:
                (_, _, claimed, got), = mark(exe, tmp, cloud.keys, R, [[v]])
                assert claimed == 1 and np.array_equal(np.sort(got), K.dirty(e, R)), (R, v)
    assert K.dirty(K.add(cloud, K.items_of_rows(cloud, rows[3:4])), 1).tolist() == [3, 4, 5]      # not the decoys 6, 7


@needs_gxx
@pytest.mark.parametrize("times", [1, 2, 1000])
def test_a_voxel_touched_many_times_is_claimed_once(exes, times):
    tmp, builds = exes
    cloud = K.Cloud.of_rows(K.sheet(300, seed=5, h=H), H)
    e = K.add(cloud, K.items_of_rows(cloud, K.cells_rows(cloud.keys[[17]], H)))
    for exe in builds:
        (_, _, claimed, got), = mark(exe, tmp, cloud.keys, 2, [[17] * times])
        assert claimed == 1 and len(got) == len(set(got.tolist())) and np.array_equal(np.sort(got), K.dirty(e, 2))


@needs_gxx
def test_the_epoch_wraps_without_losing_a_dirty_voxel(exes):
    tmp, builds = exes
    cloud = K.Cloud.of_rows(K.sheet(300, seed=6, h=H), H)
    items = [17, 18, 17, 250]
    e = K.add(cloud, K.items_of_rows(cloud, K.cells_rows(cloud.keys[items], H)))
    D = K.dirty(e, 2)
    for exe in builds:
        runs = mark(exe, tmp, cloud.keys, 2, [items] * 4, epoch=0xFFFFFFFD)
        assert [(r[0], r[1]) for r in runs] == [(0xFFFFFFFE, 0), (0xFFFFFFFF, 0), (1, 1), (2, 0)]
        for _, _, claimed, got in runs:
            assert claimed == 3 and len(got) == len(set(got.tolist())) and np.array_equal(np.sort(got), D)
        (first, cleared, _, _), = mark(exe, tmp, cloud.keys, 2, [items])       # 0 is no epoch: the first edit runs at 1
        assert (first, cleared) == (1, 0)


# ---- (3) the module surface ----------------------------------------------------------------------------------------------
NEW = ("mc_voxel_keep_normals", "mc_voxel_kept_normals", "mc_voxel_kept_info", "mc_voxel_drop_normals",
       "mc_timing_read_kept_normals")


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


def test_argument_errors_need_no_device():
    m = pkg()
    cloud = m.VoxelCloud(_NoDevice(), 10, 7, 0.05)
    for radius in (0, 0.0, -0.1, float("nan"), float("inf"), "x", 0.2005, 1.0):
        with pytest.raises(ValueError):
            cloud.keep_normals(radius)
    with pytest.raises(ValueError, match="voxelise coarser or shrink the radius"):
        cloud.keep_normals(0.2005)
    with pytest.raises(ValueError, match="radius must be finite and > 0"):
        cloud.keep_normals(-1.0)
    for max_nn in (1, 2, -1, 65, 30.0, "30", None, True):
        with pytest.raises(ValueError, match="max_nn must be 0 .no cap. or an integer in 3..64"):
            cloud.keep_normals(0.1, max_nn)
        with pytest.raises(ValueError, match="max_nn must be"):
            cloud.keep_normals(max_nn=max_nn)
    with pytest.raises(ValueError, match="twice the voxel size"):
        m.VoxelCloud(_NoDevice(), 10, 7).keep_normals()
    closed = m.VoxelCloud(_NoDevice(), 10, 6, 0.05)      # not the context's live generation
    for call in (closed.keep_normals, closed.kept_normals, closed.drop_normals, lambda: closed.kept):
        with pytest.raises(ValueError, match="closed or was replaced"):
            call()
    assert m.VoxelKept is m.voxel.VoxelKept
    assert m.VoxelKept._fields == ("radius", "max_nn", "full_passes", "refreshed_last", "refreshed_total")
    assert callable(m.Context.read_timing_kept_normals) and isinstance(m.VoxelCloud.kept, property)
    assert "keep_normals" in m.__doc__ and "Kept normals" in m.voxel.__doc__


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert "dirty set D" in hdr and "48 bytes per voxel" in hdr
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    assert lib.mc_voxel_keep_normals(None, 0.1, 30) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_kept_normals(None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_kept_info(None, None, None, None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_drop_normals(None) == m._lib.MC_ERR_INVALID
    assert lib.mc_timing_read_kept_normals(None, None, None) == m._lib.MC_ERR_INVALID
