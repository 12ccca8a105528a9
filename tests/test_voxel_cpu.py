"""The voxel-grid filter without a GPU: (1) the scalar core of csrc/voxel_core.hpp, included by
tests/host/voxel_host.cpp, built with g++ plainly and under
ASan + UBSan, and compared bit for bit with the NumPy restatement of tests/voxel.py on the boundary and
range values; (2) the restatement's own accuracy bounds against exact rational means; (3) the module
surface that needs no device."""
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import hostbuild
import voxel as V
from conftest import pkg

ROOT = hostbuild.ROOT

QUANT_OUT = np.dtype([("k", "<i4", (3,)), ("bad", "<i4"), ("Q", "<i8", (3,)), ("QI", "<i8"), ("key", "<u8"),
                      ("uk", "<i4", (3,)), ("zero", "<i4")])
FIN_IN = np.dtype([("k", "<i4", (3,)), ("zero", "<i4"), ("S", "<i8", (3,)), ("SI", "<i8"), ("n", "<i8")])
FIN_OUT = np.dtype([("c", "<f8", (4,)), ("f", "<f4", (4,))])

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("voxel_host")
    return tmp, [hostbuild.build(tmp, "voxel_host.cpp", "-ffp-contract=off", sanitize=san) for san in (False, True)]


def run(exe, tmp, mode, h, origin, body):
    src, dst = tmp / "in.bin", tmp / "out.bin"
    src.write_bytes(np.array([h, *origin], np.float64).tobytes() + body)
    hostbuild.run(exe, mode, src, dst, timeout=120)
    return dst.read_bytes()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- (1) the core under g++ ----------------------------------------------------------------------------------
def test_edge_list_holds_what_it_promises():
    """The named cases, by hand: f rounding up to exactly 1.0, both key ends and the first keys beyond
    them, the intensity ends."""
    K, Q, QI, bad = V.quantise([[-1e-20, 0.0, -0.0]], [0.5], 0.5, (0, 0, 0))
    assert K.tolist() == [[-1, 0, 0]] and Q.tolist() == [[1 << 32, 0, 0]] and QI.tolist() == [1 << 15] and not bad.any()
    h = 0.5
    rows = np.array([[-(2 ** 20) * h, (2 ** 20 - 1) * h + 0.49, 0.0, 0.0],     # both ends accepted
                     [2 ** 20 * h, 0.0, 0.0, 0.0], [0.0, (-(2 ** 20) - 1) * h, 0.0, 0.0],
                     [0.0, 0.0, np.nextafter(-(2 ** 20) * h, -np.inf), 0.0],
                     [0.0, 0.0, 0.0, 65536.0], [0.0, 0.0, 0.0, -65536.0],
                     [0.0, 0.0, 0.0, float(np.nextafter(np.float32(65536.0), np.float32(np.inf)))]])
    K, _, QI, bad = V.quantise(rows[:, :3], rows[:, 3], h, (0, 0, 0))
    assert bad.tolist() == [False, True, True, True, False, False, True]
    assert K[0].tolist() == [-(2 ** 20), 2 ** 20 - 1, 0] and QI[4] == 2 ** 32 and QI[5] == -(2 ** 32)
    for h, o in V.GRIDS:
        for dt in (np.float64, np.float32):
            acc, ref = V.edge_rows(h, o, dt)
            K, Q, _, bad = V.quantise(acc[:, :3], acc[:, 3], h, o)
            assert not bad.any() and V.quantise(ref[:, :3], ref[:, 3], h, o)[3].all()
            if dt is np.float64:
                assert K.min() == V.KEY_MIN and K.max() == V.KEY_END - 1
            if o[0] == 0.0:   # a tiny negative g: f rounds up to exactly 1.0
                assert (Q == 1 << 32).any() and (Q == 0).any()


@needs_gxx
def test_core_equals_the_restatement_bit_for_bit(exes):
    tmp, builds = exes
    rng = np.random.default_rng(20250101)
    for h, o in V.GRIDS:
        parts = []
        for dt in (np.float64, np.float32):
            parts.extend(V.edge_rows(h, o, dt))
        cloud = np.asarray(o) + rng.uniform(-40.0, 40.0, (3000, 3))
        parts.append(np.column_stack([cloud, rng.uniform(0.0, 1.0, 3000)]))
        rows = np.concatenate(parts)
        K, Q, QI, bad = V.quantise(rows[:, :3], rows[:, 3], h, o)
        assert bad.sum() >= 30 and (~bad).sum() >= 3000
        # the finaliser: the voxels of the accepted rows, then records with sums up to n * 2^32, n up to 2^31 - 1
        d = V.downsample(rows[~bad], h, o)
        n_big = rng.integers(1, 2 ** 31, 400)
        n_big[:4] = [1, 2 ** 31 - 1, 3, 2 ** 31 - 1]
        S_big = np.array([[int(rng.integers(0, int(n) * 2 ** 32 + 1)) for _ in range(3)] for n in n_big], np.int64)
        S_big[1] = int(n_big[1]) * 2 ** 32
        S_big[2] = 0
        rec = np.zeros(len(d["rows"]) + 400, FIN_IN)
        rec["k"] = np.concatenate([d["keys"], rng.integers(V.KEY_MIN, V.KEY_END, (400, 3))])
        rec["S"] = np.concatenate([d["S"], S_big])
        rec["SI"] = np.concatenate([d["SI"], rng.integers(-(2 ** 32), 2 ** 32, 400) * n_big])
        rec["n"] = np.concatenate([d["counts"].astype(np.int64), n_big])
        want = V.finalise(rec["k"], rec["S"], rec["SI"], rec["n"], h, o)
        assert np.array_equal(bits(want[:len(d["rows"])]), bits(d["rows"]))
        for exe in builds:
            got = np.frombuffer(run(exe, tmp, "quant", h, o, np.ascontiguousarray(rows).tobytes()), QUANT_OUT)
            assert len(got) == len(rows)
            assert np.array_equal(got["bad"] != 0, bad), (h, o)
            assert np.array_equal(got["k"], K) and np.array_equal(got["Q"], Q) and np.array_equal(got["QI"], QI)
            assert np.array_equal(got["key"][~bad], V.pack(K[~bad]).astype(np.uint64))
            assert np.array_equal(got["uk"], got["k"]) and (got["key"] >> np.uint64(63) == 0).all()
            fin = np.frombuffer(run(exe, tmp, "fin", h, o, rec.tobytes()), FIN_OUT)
            assert np.array_equal(bits(fin["c"]), bits(want))
            assert np.array_equal(bits(fin["f"]), bits(want.astype(np.float32)))


@needs_gxx
def test_probe_never_yields_the_no_slot_index(exes):
    """A table of 2^32 slots (2^30 < N < 2^31 points) has a slot 0xFFFFFFFF, the value that marks a refused
    point in the per-point slot array: the probe sequence must pass over it, at its start (a key hashing
    there) and when stepping (from 0xFFFFFFFE), and be the plain Fibonacci hash + linear probe elsewhere."""
    tmp, builds = exes
    C, W = 0x9E3779B97F4A7C15, 1 << 64
    inv = pow(C, -1, W)
    top = [k for k in ((t * inv) % W for t in range(W - (1 << 32), W - (1 << 32) + 4000)) if k < 1 << 63][:50]
    assert len(top) == 50 and all((k * C % W) >> 32 == 0xFFFFFFFF for k in top)      # valid keys hashing to the last slot
    rng = np.random.default_rng(7)
    keys = np.array(top + rng.integers(0, 1 << 63, 2000).tolist(), np.uint64)
    for log2cap in (6, 12, 31, 32):
        mask = (1 << log2cap) - 1
        want_first = np.array([((int(k) * C % W) >> (64 - log2cap)) & mask for k in keys.tolist()], np.uint64)
        starts = np.concatenate([want_first, [mask, mask - 1, 0, 0xFFFFFFFE & mask]]).astype(np.uint64)
        want_first[want_first == 0xFFFFFFFF] = 0
        want_next = (starts + np.uint64(1)) & np.uint64(mask)
        want_next[want_next == 0xFFFFFFFF] = 0
        body = np.array([log2cap, len(keys)], np.uint64).tobytes() + keys.tobytes() + starts.tobytes()
        for exe in builds:
            got = np.frombuffer(run(exe, tmp, "probe", 1.0, (0, 0, 0), body), np.uint32)
            first, nxt = got[:len(keys)], got[len(keys):]
            assert np.array_equal(first, want_first) and np.array_equal(nxt, want_next), log2cap
            assert not (got == 0xFFFFFFFF).any()
    assert (want_first[:50] == 0).all()      # the 2^32-slot table: those keys start at slot 0 instead


# ---- (2) the definition's accuracy ---------------------------------------------------------------------------
def ulp(x):
    return float(np.spacing(np.abs(np.float64(x))))


@pytest.mark.parametrize("h", [0.01, 0.1, 0.5])
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (5.0e6, 4.4e5, 100.0)])
def test_accuracy_against_exact_rational_means(h, origin):
    """Against fractions.Fraction means of the float64 inputs, voxels of 12 points each:
    |c - mean| <= h * 2^-32 + R, where R is the float64 rounding of the definition's own operations —
    half an ulp each of a = v - o (in metres), of g and of w = k + m 2^-32 (in voxels, times h), of
    w * h and of c; the float32 output within 1 float32 ulp of the correctly rounded mean; the intensity
    within 2^-17, and that bound is reached."""
    rng = np.random.default_rng(int(h * 1000) + int(origin[0]) % 997)
    o = np.asarray(origin, np.float64)
    nvox, per = 40, 12
    keys = rng.integers(-3000, 3000, (nvox, 3))
    keys[:6] = [[V.KEY_END - 1] * 3, [V.KEY_MIN] * 3, [V.KEY_END - 1, V.KEY_MIN, 0], [0, 0, 0], [-1, -1, -1], [1, 0, -1]]
    u = rng.uniform(0.02, 0.98, (nvox, per, 3))
    pts = o + (keys[:, None, :] + u) * h
    inten = rng.uniform(0.0, 1.0, (nvox, per))
    inten[3] = 1.5 / 65536.0          # a tie of the intensity grid in every point: the error is 2^-17 exactly
    rows = np.column_stack([pts.reshape(-1, 3), inten.reshape(-1)])
    rows = rows[rng.permutation(len(rows))]
    d = V.downsample(rows, h, o)
    assert len(d["rows"]) == nvox and (d["counts"] == per).all()
    K = V.quantise(rows[:, :3], rows[:, 3], h, o)[0]
    worst = worst_i = 0.0
    for v in range(nvox):
        sel = (K == d["keys"][v]).all(axis=1)
        assert sel.sum() == per
        for c in range(4):
            mean = sum(Fraction(float(x)) for x in rows[sel, c]) / per
            got = float(d["rows"][v, c])
            err = abs(Fraction(got) - mean)
            if c == 3:
                assert err <= Fraction(1, 2 ** 17)
                worst_i = max(worst_i, float(err))
                continue
            a_max = np.abs(rows[sel, c] - o[c]).max()
            k_abs = abs(int(d["keys"][v, c])) + 1.0
            R = (ulp(a_max) + h * ulp(a_max / h) + h * ulp(k_abs) + ulp(k_abs * h) + ulp(got)) / 2
            assert err <= Fraction(h) / 2 ** 32 + Fraction(R), (v, c, float(err) / h)
            worst = max(worst, float(err) / h)
            m32 = np.float32(float(mean))
            assert abs(float(d["f32"][v, c]) - float(m32)) <= float(np.spacing(np.abs(m32)))
    print(f"h {h} origin {origin}: worst |c - mean| = {worst:.3e} h, worst intensity error {worst_i:.3e}")
    assert worst_i == 2.0 ** -17


# ---- (3) the module surface --------------------------------------------------------------------------------
NEW = ("mc_voxel_build_batch", "mc_voxel_build_f64", "mc_voxel_emit_batch", "mc_voxel_emit_f64", "mc_timing_read_voxel",
       "mc_voxel_release")


def test_argument_errors_need_no_device():
    m = pkg()
    rows = np.zeros((5, 4))
    for bad in (0, 0.0, -0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            m.voxel_downsample(rows, bad)
    for origin in ((0, 0), (0, 0, float("nan")), (0, float("inf"), 0), 1.0):
        with pytest.raises(ValueError):
            m.voxel_downsample(rows, 0.1, origin)
    for shape in ((5, 3), (5,), (2, 2, 4)):
        with pytest.raises(ValueError):
            m.voxel_downsample(np.zeros(shape), 0.1)
    assert callable(m.Context.voxel_downsample) and m.VoxelCloud is m.voxel.VoxelCloud
    for name in ("n_voxels", "batch", "rows", "point_counts", "keys", "close"):
        assert name == "n_voxels" or callable(getattr(m.VoxelCloud, name))


def test_symbols_exported_and_abi_unchanged():
    m = pkg()
    lib = m._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mcdeskew.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mc_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared and name in m._lib.EXPORTED and hasattr(lib, name), name
    assert re.search(r"^#define MC_ABI_VERSION 1$", hdr, flags=re.M) and lib.mc_abi_version() == 1
    # the library refuses the same arguments itself (no context is needed to be told so)
    n = m._lib.c_int64(0)
    o = np.zeros(3)
    p = m._lib.ptr(o, m._lib.c_double)
    assert lib.mc_voxel_build_f64(None, None, 4, 0, 0.1, p, m._lib.ctypes.byref(n), None) == m._lib.MC_ERR_INVALID
    assert lib.mc_voxel_emit_f64(None, None, None, None) == m._lib.MC_ERR_INVALID
