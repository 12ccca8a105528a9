"""Shrinking a voxel cloud without a GPU: (1) the restatement of tests/voxelremove.py against the one-shot restatement
of tests/voxel.py: remove, insert then subtract, the remainder of A ++ B minus A, and every refusal; (2) the shrink rule
and the remainder check of csrc/voxel_core.hpp, compiled with g++ by tests/host/voxel_remove_host.cpp, against the
restatement on both sides of every edge; (3) the module surface that needs no device."""
import os
import re
import shutil
import types

import numpy as np
import pytest

import hostbuild
import voxel as V
import voxelinsert as VI
import voxelremove as VR
from conftest import pkg

ROOT = hostbuild.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
FIELDS = ("rows", "counts", "keys", "f32", "S", "SI")


def same(got, want, order=None):
    for f in FIELDS:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if order is not None:
            a, b = np.ascontiguousarray(a[order[0]]), np.ascontiguousarray(b[order[1]])
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tobytes() == b.tobytes(), f


def by_key(d):
    return np.argsort(V.pack(d["keys"]), kind="stable")


def source(seed, n=6000, h=0.2):
    rng = np.random.default_rng(seed)
    centre = rng.integers(-20, 20, (900, 3))
    pick = rng.integers(0, 900, n)
    return np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (n, 3))) * h, rng.uniform(-3, 3, n)])


def grid_source(seed):
    h, origin = V.GRIDS[seed % len(V.GRIDS)]
    return h, origin, source(seed, h=h) + np.array([*origin, 0.0])


def voxel_of(rows, h, origin):
    return V.pack(V.quantise(rows[:, :3], rows[:, 3], h, origin)[0])


# ---- (1) the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_remove_equals_the_one_shot_cloud_of_the_rows_left(seed):
    h, origin, rows = grid_source(seed)
    rng = np.random.default_rng(200 + seed)
    M = len(V.downsample(rows, h, origin)["keys"])
    for mask in (np.zeros(M, np.bool_), np.ones(M, np.bool_), np.arange(M) % 2 == 0, rng.random(M) < 0.1, rng.random(M) < 0.9):
        c = VR.Cloud(h, origin)
        cut = len(rows) // 3
        c.insert(rows[:cut])
        c.insert(rows[cut:])
        gone = V.pack(c.keys[mask])
        assert c.remove(mask) == int(mask.sum())
        left = rows[~np.isin(voxel_of(rows, h, origin), gone)]
        same(c.result(), V.downsample(left, h, origin))
        assert c.N == len(left)
    c.insert(rows)                                      # what is left takes more
    assert c.N == len(left) + len(rows)


@pytest.mark.parametrize("seed", range(6))
def test_insert_then_subtract_is_the_identity(seed):
    h, origin, rows = grid_source(seed)
    rng = np.random.default_rng(300 + seed)
    for _ in range(4):
        a, b = np.sort(rng.integers(0, len(rows) + 1, 2))
        base, extra = np.concatenate([rows[:a], rows[b:]]), rows[a:b]         # extra shares some voxels and brings others
        c = VR.Cloud(h, origin)
        c.insert(base)
        before, N = c.result(), c.N
        grown = c.insert(extra)
        assert c.subtract(extra) == grown and c.N == N
        same(c.result(), before)
        grown = c.merge(*VI.records_of(V.downsample(extra, h, origin))) if len(extra) else 0
        assert (c.subtract_records(*VI.records_of(V.downsample(extra, h, origin))) if len(extra) else 0) == grown and c.N == N
        same(c.result(), before)


@pytest.mark.parametrize("seed", range(6))
def test_the_remainder_of_a_cloud_minus_its_head(seed):
    h, origin, rows = grid_source(seed)
    rng = np.random.default_rng(400 + seed)
    for cut in (0, 1, int(rng.integers(1, len(rows))), len(rows) - 1, len(rows)):
        A, B = rows[:cut], rows[cut:]
        c = VR.Cloud(h, origin)
        c.insert(rows)
        order_before = V.pack(c.keys)
        M = len(c.keys)
        want = V.downsample(B, h, origin)
        assert c.subtract(A) == M - len(want["keys"]) and c.N == len(B)
        got = c.result()
        same(got, want, (by_key(got), by_key(want)))
        # the relative order the survivors had, which a build of B alone need not give them
        assert np.array_equal(V.pack(c.keys), order_before[np.isin(order_before, V.pack(want["keys"]))])
        # the same by records, in one call and key by key
        r = VR.Cloud(h, origin)
        r.insert(rows)
        if cut:
            r.subtract_records(*VI.records_of(V.downsample(A, h, origin)))
        same(r.result(), got)


def refusal(call, index, reason):
    with pytest.raises(V.Refused) as e:
        call()
    assert (e.value.index, e.value.reason) == (index, reason)
    return e.value


def test_every_refusal_changes_nothing():
    h = 0.2
    rows = source(9)
    c = VR.Cloud(h)
    c.insert(rows[:3000])
    before, N = c.result(), c.N
    # an item the filter refuses, and the lowest of several
    bad = rows[:1000].copy()
    bad[400, 3] = 65537.0
    bad[17, 1] = np.nan
    refusal(lambda: c.subtract(bad), 17, VR.ITEM)
    # a voxel the cloud lacks: the lowest, and before a later NaN
    away = rows[:1000].copy()
    away[[50, 60], 0] += 1000.0
    away[70, 2] = np.inf
    refusal(lambda: c.subtract(away), 50, VR.MISSING)
    away[20, 0] = np.nan
    refusal(lambda: c.subtract(away), 20, VR.ITEM)
    # more points than the cloud holds
    refusal(lambda: c.subtract(np.concatenate([rows[:3000], rows[:1]])), -1, VR.POINTS)
    # one more point of a voxel than it holds: the lowest item of that voxel
    vox = voxel_of(rows[:3000], h, V.ZERO)
    v = vox[5]
    mine = rows[:3000][vox == v]
    other = rows[:3000][vox != v][:3]
    e = refusal(lambda: c.subtract(np.concatenate([other, mine, mine[:1]])), 3, VR.REMAINDER)
    assert V.pack(np.array([e.key]))[0] == v
    # counts that fit, a sum that cannot: two points at a voxel's low corner minus one near its high corner
    two = VR.Cloud(h)
    two.insert(np.array([[0.01, 0.01, 0.01, 0.0], [0.02, 0.02, 0.02, 0.0], [5.0, 5.0, 5.0, 1.0]]))
    kept = two.result()
    e = refusal(lambda: two.subtract(np.array([[5.0, 5.0, 5.0, 1.0], [0.19, 0.19, 0.19, 0.0]])), 1, VR.REMAINDER)
    assert e.key == (0, 0, 0)
    same(two.result(), kept)
    assert two.N == 3
    # records: a bad one, a missing one, a count of 0 left with a sum
    k, n, S, SI = VI.records_of(V.downsample(rows[:1000], h))
    n0 = n.copy()
    n0[5] = 0
    refusal(lambda: c.subtract_records(k, n0, S, SI), 5, VR.ITEM)
    k1 = k.copy()
    k1[7] += 5000
    refusal(lambda: c.subtract_records(k1, n, S, SI), 7, VR.MISSING)
    full = VI.records_of(before)
    S1 = full[2].copy()
    S1[9, 0] -= 1
    refusal(lambda: c.subtract_records(full[0], full[1], S1, full[3]), 9, VR.REMAINDER)
    same(c.result(), before)
    assert c.N == N
    # an empty cloud holds no voxel; an empty call is nothing
    empty = VR.Cloud(h)
    assert empty.subtract(np.zeros((0, 4))) == 0
    refusal(lambda: empty.subtract(rows[:2]), 0, VR.MISSING)
    # and the whole cloud leaves
    assert c.subtract_records(*full) == len(before["keys"]) and c.N == 0 and len(c.keys) == 0
    c.insert(rows[:100])
    same(c.result(), V.downsample(rows[:100], h))


# ---- (2) the scalar rules as the device compiles them ----------------------------------------------------------------
def shrink_cases():
    out = [(0, 0), (5, 0)]
    for log2cap in (6, 7, 9, 12, 13, 20, 27, 31, 32):
        eighth = (1 << log2cap) // 8
        for M in (eighth - 1, eighth, eighth + 1, 0, 1, 15, 16, 17, eighth // 2, eighth // 4, eighth // 4 + 1, 4 * eighth):
            if M >= 0:
                out.append((M, log2cap))
    return out


def remainder_cases():
    top = lambda n: n << 32                                                    # noqa: E731
    out = [(-1, (0, 0, 0), 0), (-1, (5, 5, 5), 5), (-2 ** 31, (0, 0, 0), 0), (2 ** 31, (0, 0, 0), 0), (0, (0, 0, 0), 0)]
    for c in range(3):
        for s in (1, -1, 1 << 40):
            S = [0, 0, 0]
            S[c] = s
            out.append((0, S, 0))
    out += [(0, (0, 0, 0), 1), (0, (0, 0, 0), -1)]
    for n in (1, 2, 7, 2 ** 30 - 1, 2 ** 31 - 1):
        for s in (0, 1, -1, top(n) - 1, top(n), top(n) + 1):
            for c in range(3):
                S = [5, 5, 5]
                S[c] = s
                out.append((n, S, 0))
        for si in (0, top(n), -top(n), top(n) + 1, -(top(n) + 1)):
            out.append((n, (0, top(n), 1), si))
    return out


@needs_gxx
def test_shrink_rule_and_remainder_check_as_compiled(tmp_path):
    shrinks, rems = shrink_cases(), remainder_cases()
    # the edges the rules are pinned on, by hand
    assert VR.table_shrink_log2(512, 12) == 12 and VR.table_shrink_log2(511, 12) == 11 and VR.table_shrink_log2(513, 12) == 12
    assert VR.table_shrink_log2(256, 12) == 10 and VR.table_shrink_log2(257, 12) == 11 and VR.table_shrink_log2(0, 12) == 6
    assert VR.table_shrink_log2(1, 12) == 6 and VR.table_shrink_log2(16, 12) == 6 and VR.table_shrink_log2(17, 12) == 7
    assert VR.table_shrink_log2(7, 6) == 6 and VR.table_shrink_log2(0, 6) == 6 and VR.table_shrink_log2(0, 0) == 0
    assert VR.table_shrink_log2(2 ** 29 - 1, 32) == 31 and VR.table_shrink_log2(2 ** 29, 32) == 32
    assert VR.remainder_ok(0, (0, 0, 0), 0) and not VR.remainder_ok(0, (0, 1, 0), 0) and not VR.remainder_ok(0, (0, 0, 0), -1)
    assert not VR.remainder_ok(-1, (0, 0, 0), 0) and VR.remainder_ok(1, (0, 1 << 32, 0), -(1 << 32))
    assert not VR.remainder_ok(1, (0, (1 << 32) + 1, 0), 0) and not VR.remainder_ok(1, (-1, 0, 0), 0)
    assert not VR.remainder_ok(2, (0, 0, 0), (2 << 32) + 1) and not VR.remainder_ok(2, (0, 0, 0), -(2 << 32) - 1)
    # a shrunk table never grows, stays a quarter full at most, and a kept one is at least an eighth full
    for M, l in shrinks:
        got = VR.table_shrink_log2(M, l)
        assert got <= l and (got == l or (4 * M <= (1 << got) and (got == VI.LOG2_MIN or 4 * M > (1 << (got - 1)))))
    lines = [f"s {M} {l}" for M, l in shrinks]
    lines += ["m " + " ".join(str(int(v)) for v in (n, *S, SI)) for n, S, SI in rems]
    want = [VR.table_shrink_log2(*s) for s in shrinks] + [int(VR.remainder_ok(*r)) for r in rems]
    assert 0 in want[len(shrinks):] and 1 in want[len(shrinks):]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    for san in (False, True):
        exe = hostbuild.build(tmp_path, "voxel_remove_host.cpp", "-ffp-contract=off", sanitize=san)
        got = [int(v) for v in hostbuild.run(exe, cases).stdout.split()]
        assert len(got) == len(want)
        for line, g, w in zip(lines, got, want):
            assert g == w, (line, g, w)


# ---- (3) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_remove", "mc_voxel_subtract_batch", "mc_voxel_subtract_f64", "mc_voxel_subtract_sums",
       "mc_timing_read_voxel_remove")


def test_symbols_exported_and_refuse_null_without_a_context():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    for k, name in enumerate(("OK", "ITEM", "MISSING", "POINTS", "REMAINDER")):
        assert re.search(rf"^#define MC_VOXEL_SUB_{name} {k}$", hdr, flags=re.M), name
    assert [VR.WHY[r] for r in (VR.ITEM, VR.MISSING, VR.POINTS, VR.REMAINDER)] == [1, 2, 3, 4]
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    n, b, w = m._lib.c_int64(0), m._lib.c_int64(0), m._lib.c_int32(0)
    ref = m._lib.ctypes.byref
    bad = m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_remove(None, None, ref(n)) == bad
    assert lib.mc_voxel_subtract_batch(None, None, ref(n), None, None, ref(w)) == bad
    assert lib.mc_voxel_subtract_f64(None, None, 4, 0, ref(n), ref(b), ref(w)) == bad
    assert lib.mc_voxel_subtract_sums(None, None, None, None, 0, ref(n), ref(b), ref(w)) == bad
    assert lib.mc_timing_read_voxel_remove(None, None, ref(n)) == bad
    assert b"NULL" in lib.mc_last_error()


def by_hand(m, n_points=10):
    """A VoxelCloud on no device: whatever reaches the library here fails on the context that is none."""
    ctx = types.SimpleNamespace(_voxel_gen=1, lib=None, handle=None)
    return m.VoxelCloud(ctx, 3, 1, 0.1, (0.0, 0.5, 0.0), n_points)


def test_the_surface_exists_and_argument_errors_need_no_device():
    m = pkg()
    for name in ("remove", "subtract"):
        assert callable(getattr(m.VoxelCloud, name)), name
    assert callable(m.Context.read_timing_voxel_remove)
    assert "remove" in m.voxel.__doc__ and "subtract" in m.voxel.__doc__ and "caller's contract" in m.VoxelCloud.subtract.__doc__
    cloud = by_hand(m)
    for mask in (np.zeros(2, np.bool_), np.zeros((3, 1), np.bool_), np.zeros(3, np.uint8), [False] * 3, None):
        with pytest.raises(ValueError, match="bool array of shape"):
            cloud.remove(mask)
    for rows in (np.zeros((5, 3)), np.zeros(5), "x", None):
        with pytest.raises(ValueError):
            cloud.subtract(rows)
    state = m.VoxelSums(np.zeros((2, 3), np.int32), np.ones(2, np.int32), np.zeros((2, 4), np.int64), 0.1, np.array([0.0, 0.5, 0.0]))
    for s in (state._replace(voxel=float(np.nextafter(0.1, 1.0))), state._replace(origin=np.zeros(3)),
              state._replace(counts=np.ones(2, np.int64)), state._replace(sums=np.zeros((2, 3), np.int64))):
        with pytest.raises(ValueError):
            cloud.subtract(s)
    closed = by_hand(m)
    closed.ctx._voxel_gen = 2
    for call in (lambda: closed.remove(np.zeros(3, np.bool_)), lambda: closed.subtract(np.zeros((1, 4))), lambda: closed.subtract(state)):
        with pytest.raises(ValueError, match="closed or was replaced"):
            call()
