"""Growing a voxel cloud without a GPU: (1) the restatement of tests/voxelinsert.py against the one-shot
restatement of tests/voxel.py; (2) the growth rule and the record check of csrc/voxel_core.hpp, compiled with g++ by
tests/host/voxel_insert_host.cpp, against the restatement on both sides of every edge; (3) the content-keeping growth
of a buffer (csrc/devbuf.hpp) as a stand-alone program under ASan + UBSan; (4) the module surface that needs no
device."""
import os
import pickle
import re
import shutil
import types

import numpy as np
import pytest

import hostbuild
import voxel as V
import voxelinsert as VI
from conftest import pkg

ROOT = hostbuild.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
FIELDS = ("rows", "counts", "keys", "f32", "S", "SI")


def same(got, want):
    for f in FIELDS:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tobytes() == b.tobytes(), f


def source(seed, n=6000, h=0.2):
    rng = np.random.default_rng(seed)
    centre = rng.integers(-20, 20, (900, 3))
    pick = rng.integers(0, 900, n)
    return np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (n, 3))) * h, rng.uniform(-3, 3, n)])


# ---- (1) the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_random_splits_equal_the_one_shot_cloud(seed):
    h, origin = V.GRIDS[seed % len(V.GRIDS)]
    rows = source(seed, h=h) + np.array([*origin, 0.0])
    whole = V.downsample(rows, h, origin)
    rng = np.random.default_rng(100 + seed)
    for parts in range(1, 8):
        cuts = np.sort(rng.integers(0, len(rows) + 1, parts - 1))        # empty parts happen
        pieces = np.split(rows, cuts)
        c, m = VI.Cloud(h, origin), VI.Cloud(h, origin)
        grown = 0
        for piece in pieces:
            before = c.keys.copy()
            grown += c.insert(piece)
            assert np.array_equal(c.keys[:len(before)], before) and len(c.keys) == grown      # ids are stable
            m.merge(*VI.records_of(V.downsample(piece, h, origin)))
        same(c.result(), whole)
        same(m.result(), whole)
        assert c.N == m.N == len(rows)


def test_a_refused_call_changes_nothing():
    rows = source(9)
    c = VI.Cloud(0.2)
    c.insert(rows[:1000])
    before = c.result()
    bad = rows[1000:2000].copy()
    bad[17, 1] = np.nan
    bad[400, 3] = 65537.0
    with pytest.raises(V.Refused) as e:
        c.insert(bad)
    assert e.value.index == 17
    same(c.result(), before)
    k, n, S, SI = VI.records_of(V.downsample(rows[1000:2000], 0.2))
    n = n.copy()
    n[5] = 0
    with pytest.raises(V.Refused) as e:
        c.merge(k, n, S, SI)
    assert e.value.index == 5 and c.N == 1000
    same(c.result(), before)
    # a key that repeats in a merge is two items of one voxel
    part = rows[1000:1500]
    k2, n2, S2, SI2 = (np.concatenate([a, a[:3]]) for a in VI.records_of(V.downsample(part, 0.2)))
    c.merge(k2, n2, S2, SI2)
    again = part[np.isin(V.pack(V.quantise(part[:, :3], part[:, 3], 0.2, V.ZERO)[0]), V.pack(k2[:3]))]     # those voxels' points
    same(c.result(), V.downsample(np.concatenate([rows[:1500], again]), 0.2))
    # the limit
    big = VI.Cloud(1.0)
    rec = (np.zeros((1, 3), np.int64), np.array([LIMIT_HALF]), np.full((1, 3), LIMIT_HALF << 32), np.array([0]))
    big.merge(*rec)
    big.merge(*rec)
    assert big.N == 2 ** 31 - 2
    with pytest.raises(ValueError):
        big.merge(*rec)
    big.insert(np.array([[0.5, 0.5, 0.5, 0.0]]))
    with pytest.raises(ValueError):
        big.insert(np.array([[0.5, 0.5, 0.5, 0.0]]))
    assert big.N == 2 ** 31 - 1 and big.n.tolist() == [2 ** 31 - 1]


LIMIT_HALF = 2 ** 30 - 1


# ---- (2) the scalar rules as the device compiles them ----------------------------------------------------------------
def grow_cases():
    out = []
    for log2cap in (6, 7, 12, 13, 20, 31, 32):
        half = (1 << log2cap) // 2
        for M in (0, 1, half // 2, half - 1):
            for n in (half - M - 1, half - M, half - M + 1, 2 * half - M, 2 * half - M + 1, 4 * half):      # M + n around cap / 2 and cap
                if n >= 0:
                    out.append((M, n, log2cap))
    out += [(0, 1, 0), (0, 32, 0), (0, 33, 0), (0, 2048, 0), (0, 2049, 0), (5, 0, 0), (0, 2 ** 31 - 1, 0), (2 ** 31 - 2, 1, 32),
            (2 ** 31 - 2, 2 ** 31 - 1, 32), (2048, 1, 12), (1024, 1024, 12), (2048, 6000, 13), (2049, 6000, 13)]
    return out


def record_cases():
    top = lambda n: n << 32                                                    # noqa: E731
    out = []
    for n in (1, 7, 2 ** 30 - 1, 2 ** 31 - 1):
        for s in (0, 1, top(n) - 1, top(n), top(n) + 1, -1):
            for c in range(3):
                S = [5, 5, 5]
                S[c] = s
                out.append(((0, 0, 0), n, S, 0))
        for si in (0, top(n), -top(n), top(n) + 1, -top(n) - 1):
            out.append(((1, -1, 2), n, (0, top(n), 1), si))
    for n in (0, -1, -2 ** 31, 2 ** 31, 2 ** 40):
        out.append(((0, 0, 0), n, (0, 0, 0), 0))
    for k in (V.KEY_MIN, V.KEY_MIN - 1, V.KEY_END - 1, V.KEY_END, -2 ** 31, 2 ** 31 - 1):
        for c in range(3):
            key = [3, -4, 5]
            key[c] = k
            out.append((key, 2, (1, 2, 3), -4))
    return out


@needs_gxx
def test_growth_rule_and_record_check_as_compiled(tmp_path):
    grows, recs = grow_cases(), record_cases()
    # the edges the rule is pinned on, by hand
    assert VI.table_log2(2048, 1, 12) == 13 and VI.table_log2(1024, 1024, 12) == 12 and VI.table_log2(2048, 0, 12) == 12
    assert VI.table_log2(2049, 6000, 13) == 14 and VI.table_log2(8049, 30000, 14) == 17 and VI.table_log2(0, 1, 0) == 6 and VI.table_log2(0, 33, 0) == 7
    assert VI.table_log2(2 ** 31 - 2, 2 ** 31 - 1, 32) == 32 and VI.table_log2(0, 2 ** 31 - 1, 0) == 32
    assert VI.record_ok((0, 0, 0), 1, (0, 1 << 32, 0), -(1 << 32)) and not VI.record_ok((0, 0, 0), 1, (0, (1 << 32) + 1, 0), 0)
    assert not VI.record_ok((0, 0, 0), 0, (0, 0, 0), 0) and not VI.record_ok((0, 0, 0), 1, (-1, 0, 0), 0)
    assert VI.record_ok((V.KEY_MIN, V.KEY_END - 1, 0), 1, (0, 0, 0), 0) and not VI.record_ok((0, V.KEY_END, 0), 1, (0, 0, 0), 0)
    lines = [f"g {M} {n} {l}" for M, n, l in grows]
    lines += ["r " + " ".join(str(int(v)) for v in (*k, n, *S, SI)) for k, n, S, SI in recs]
    want = [VI.table_log2(*g) for g in grows] + [int(VI.record_ok(*r)) for r in recs]
    assert 0 in want[len(grows):] and 1 in want[len(grows):]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    for san in (False, True):
        exe = hostbuild.build(tmp_path, "voxel_insert_host.cpp", "-ffp-contract=off", sanitize=san)
        got = [int(v) for v in hostbuild.run(exe, cases).stdout.split()]
        assert len(got) == len(want)
        for line, g, w in zip(lines, got, want):
            assert g == w, (line, g, w)


# ---- (3) the buffer that grows and keeps its contents --------------------------------------------------------------
@needs_gxx
def test_content_keeping_growth_under_asan_ubsan(tmp_path):
    exe = hostbuild.build(tmp_path, "devbuf_keep_host.cpp", "-DMC_DEVBUF_HOST_TEST", sanitize=True)
    assert hostbuild.run(exe).stdout.strip().endswith("bad 0")


# ---- (4) the module surface ----------------------------------------------------------------------------------------
NEW = ("mc_voxel_insert_batch", "mc_voxel_insert_f64", "mc_voxel_emit_sums", "mc_voxel_merge_sums", "mc_voxel_points",
       "mc_voxel_table", "mc_timing_read_voxel_insert")


def test_symbols_exported_and_refuse_null_without_a_context():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    n, b = m._lib.c_int64(0), m._lib.c_int64(0)
    ref = m._lib.ctypes.byref
    bad = m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_insert_batch(None, None, ref(n), None, None) == bad
    assert lib.mc_voxel_insert_f64(None, None, 4, 0, ref(n), ref(b)) == bad
    assert lib.mc_voxel_emit_sums(None, None) == bad
    assert lib.mc_voxel_merge_sums(None, None, None, None, 0, ref(n), ref(b)) == bad
    assert lib.mc_voxel_points(None, ref(n)) == bad
    assert lib.mc_voxel_table(None, ref(n), ref(b)) == bad
    assert lib.mc_timing_read_voxel_insert(None, None, ref(n)) == bad
    assert b"NULL" in lib.mc_last_error()


def by_hand(m, n_points=10):
    """A VoxelCloud on no device: whatever reaches the library here fails on the context that is none."""
    ctx = types.SimpleNamespace(_voxel_gen=1, lib=None, handle=None)
    return m.VoxelCloud(ctx, 3, 1, 0.1, (0.0, 0.5, 0.0), n_points)


def good_state(m, **kw):
    s = dict(keys=np.zeros((2, 3), np.int32), counts=np.ones(2, np.int32), sums=np.zeros((2, 4), np.int64), voxel=0.1,
             origin=np.array([0.0, 0.5, 0.0]))
    s.update(kw)
    return m.VoxelSums(**s)


def test_the_surface_exists():
    m = pkg()
    assert m.VoxelSums is m.voxel.VoxelSums and m.VoxelSums._fields == ("keys", "counts", "sums", "voxel", "origin")
    for name in ("insert", "merge", "state"):
        assert callable(getattr(m.VoxelCloud, name)), name
    assert by_hand(m).n_points == 10 and callable(m.Context.read_timing_voxel_insert)
    s = pickle.loads(pickle.dumps(good_state(m)))
    assert isinstance(s, m.VoxelSums) and s.voxel == 0.1 and s.keys.dtype == np.int32
    assert "insert" in m.voxel.__doc__ and "merge" in m.voxel.__doc__


def test_argument_errors_need_no_device():
    m = pkg()
    cloud = by_hand(m)
    for rows in (np.zeros((5, 3)), np.zeros(5), np.zeros((2, 2, 4)), "x", None, np.array([["a"] * 4])):
        with pytest.raises(ValueError):
            cloud.insert(rows)
    full = by_hand(m, n_points=2 ** 31 - 3)
    with pytest.raises(ValueError, match="2\\^31"):
        full.insert(np.zeros((3, 4)))
    one = np.nextafter(0.1, 1.0)
    states = [good_state(m, voxel=one), good_state(m, voxel=np.float64(-0.1)), good_state(m, voxel="0.1"),
              good_state(m, origin=np.array([0.0, np.nextafter(0.5, 0.0), 0.0])), good_state(m, origin=np.array([-0.0, 0.5, 0.0])),
              good_state(m, origin=(0.0, 0.5, 0.0)), good_state(m, origin=np.zeros(2)), good_state(m, origin=np.zeros(3, np.float32)),
              good_state(m, keys=np.zeros((2, 3), np.int64)), good_state(m, keys=np.zeros((2, 4), np.int32)),
              good_state(m, keys=np.zeros(6, np.int32)), good_state(m, counts=np.ones(2, np.int64)),
              good_state(m, counts=np.ones((2, 1), np.int32)), good_state(m, counts=np.ones(3, np.int32)),
              good_state(m, sums=np.zeros((2, 4), np.float64)), good_state(m, sums=np.zeros((2, 3), np.int64)),
              good_state(m, sums=np.zeros((1, 4), np.int64)), good_state(m, sums=[[0] * 4] * 2),
              (np.zeros((2, 3), np.int32),), None, "state"]
    for s in states:
        with pytest.raises(ValueError):
            cloud.merge(s)
    # a cloud that does not know its grid takes no records
    bare = m.VoxelCloud(types.SimpleNamespace(_voxel_gen=1), 3, 1)
    with pytest.raises(ValueError):
        bare.merge(good_state(m))
    # a closed cloud says so before anything else happens
    closed = by_hand(m)
    closed.ctx._voxel_gen = 2
    for call in (lambda: closed.insert(np.zeros((1, 4))), lambda: closed.merge(good_state(m)), closed.state):
        with pytest.raises(ValueError, match="closed or was replaced"):
            call()
