"""The voxel-grid filter restated in NumPy: this project's own definition (include/mcdeskew.h
"voxel-grid downsampling"), which the kernels of csrc/voxel.hpp must reproduce bit for bit.

Every line of float64 arithmetic below is one IEEE operation on arrays; the sums are int64."""
import numpy as np

KEY_MIN, KEY_END = -(1 << 20), 1 << 20
FRAC = 4294967296.0          # 2^32
INT = 65536.0                # 2^16


def quantise(xyz, intensity, h, origin):
    """-> k (N, 3) int64, Q (N, 3) int64, QI (N,) int64, bad (N,) bool; refused points hold zeros."""
    v = np.asarray(xyz, np.float64).reshape(-1, 3)
    it = np.asarray(intensity, np.float64).reshape(-1)
    o = np.asarray(origin, np.float64).reshape(3)
    h = np.float64(h)
    with np.errstate(all="ignore"):
        a = v - o
        g = a / h
        k = np.floor(g)
        f = g - k
        ok = np.isfinite(v) & np.isfinite(g) & (k >= KEY_MIN) & (k < KEY_END)
        q = np.rint(f * FRAC)
        iok = np.isfinite(it) & (np.abs(it) <= INT)
        qi = np.rint(it * INT)
    bad = ~(ok.all(axis=1) & iok)
    good = ~bad
    K = np.zeros(v.shape, np.int64)
    Q = np.zeros(v.shape, np.int64)
    QI = np.zeros(len(v), np.int64)
    K[good] = k[good].astype(np.int64)
    Q[good] = q[good].astype(np.int64)
    QI[good] = qi[good].astype(np.int64)
    return K, Q, QI, bad


def pack(k):
    k = np.asarray(k, np.int64) - KEY_MIN
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def finalise(k, S, SI, n, h, origin):
    """-> (M, 4) float64 cx, cy, cz, intensity."""
    o = np.asarray(origin, np.float64).reshape(3)
    h = np.float64(h)
    dn = np.asarray(n).astype(np.float64)
    out = np.empty((len(dn), 4), np.float64)
    m = np.asarray(S, np.int64).astype(np.float64) / dn[:, None]
    s = m * (1.0 / FRAC)
    w = np.asarray(k, np.int64).astype(np.float64) + s
    t = w * h
    out[:, :3] = o + t
    mi = np.asarray(SI, np.int64).astype(np.float64) / dn
    out[:, 3] = mi * (1.0 / INT)
    return out


class Refused(ValueError):
    def __init__(self, index):
        super().__init__(f"point {index} refused")
        self.index = index


def downsample(rows, h, origin=(0.0, 0.0, 0.0)):
    """rows (N, >= 4) float64 in index order -> dict(rows (M, 4) f64, counts (M,) i32, keys (M, 3) i32,
    f32 (M, 4) float32, S (M, 3) i64, SI (M,) i64); raises Refused(lowest refused index)."""
    rows = np.asarray(rows, np.float64)
    K, Q, QI, bad = quantise(rows[:, :3], rows[:, 3], h, origin)
    if bad.any():
        raise Refused(int(np.flatnonzero(bad)[0]))
    if len(rows) == 0:
        z = np.zeros
        return dict(rows=z((0, 4)), counts=z(0, np.int32), keys=z((0, 3), np.int32), f32=z((0, 4), np.float32),
                    S=z((0, 3), np.int64), SI=z(0, np.int64))
    _, first, inv = np.unique(pack(K), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")          # voxels by their first point
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    vid = rank[inv]
    M = len(first)
    S = np.zeros((M, 3), np.int64)
    SI = np.zeros(M, np.int64)
    n = np.zeros(M, np.int64)
    np.add.at(S, vid, Q)
    np.add.at(SI, vid, QI)
    np.add.at(n, vid, 1)
    keys = K[first[order]]
    out = finalise(keys, S, SI, n, h, origin)
    return dict(rows=out, counts=n.astype(np.int32), keys=keys.astype(np.int32), f32=out.astype(np.float32), S=S, SI=SI)


# ---- the boundary and range values (tests/test_voxel_cpu.py on the host core, tests/test_gpu_voxel.py
# on the kernels) ---------------------------------------------------------------------------------------
GRIDS = ((0.5, (0.0, 0.0, 0.0)),                       # h exact in binary
         (0.1, (0.0, 0.0, 0.0)),                       # h inexact
         (0.1, (5.0e6, 4.4e5, 100.0)))                 # a UTM-scale origin


# ---- the grids off the default origin that every analysis of the voxel cloud runs on (tests/normals.py,
# clusters.py, planes.py and registration.py build their grid cases on these; the test files of the four analyses
# are parametrized over the names) ----------------------------------------------------------------------------
ZERO = (0.0, 0.0, 0.0)
# name: h, origin, moved (the cloud and the sources are moved by the origin), batch (float32 can hold the case)
ORIGIN_GRIDS = {
    # GRIDS' own UTM-scale origin, the cloud there: o + k h is dominated by o; float32 cannot resolve h
    "utm": dict(h=0.2, origin=GRIDS[2][1], moved=True, batch=False),
    # an origin that is no multiple of h on any axis: a cell's faces are not where the default grid has them
    "fractional": dict(h=0.2, origin=(0.1, -0.37, 12.3456), moved=False, batch=True),
    # the cloud stays near zero and the origin is far: keys near (825 000, -500 000, 250 000), in range, and
    # o + k h cancels down to the cloud's small coordinates
    "far keys": dict(h=0.4, origin=(-3.3e5 + 0.1, 2.0e5 + 0.07, -1.0e5 - 0.03), moved=False, batch=True),
    # the same with a voxel size that is far from a power of two
    "far keys, coarse": dict(h=7.3, origin=(5.0e6, -4.4e6, 3.0e6), moved=False, batch=False),
}


def on_grid(points, grid):
    """points (n, >= 3) where the grid has its cloud: moved by the origin for a moved grid, else as they are."""
    g = ORIGIN_GRIDS[grid]
    out = np.array(points, np.float64)
    if g["moved"]:
        out[:, :3] = out[:, :3] + np.asarray(g["origin"], np.float64)
    return out


def as_float32(rows):
    """The rows a batch can hold: every value rounded to float32, as float64."""
    return np.asarray(rows, np.float64).astype(np.float32).astype(np.float64)


def edge_rows(h, origin, dtype=np.float64):
    """-> (accepted rows, refused rows) of the grid's boundary and range values; ``dtype`` float32: the
    values a batch can hold (1 ulp is then a float32 ulp)."""
    o = np.asarray(origin, np.float64)
    inf = np.inf
    acc, ref = [], []
    for c in range(3):
        other = (o + 0.25 * h).astype(dtype).astype(np.float64)
        ks = np.array([0, 1, -1, 2, 7, -7, 1000, -1000, 123457, -123457, KEY_END - 1, KEY_MIN, KEY_MIN + 1], np.float64)
        at = (o[c] + ks * h).astype(dtype)
        vals = np.concatenate([at, np.nextafter(at, dtype(-inf)), np.nextafter(at, dtype(inf)),
                               (o[c] + np.array([-0.0, 0.0, 1e-300, -1e-300, -1e-20 * h, 0.5 * h])).astype(dtype)])
        if o[c] == 0.0:
            vals = np.concatenate([vals, np.array([-0.0, 1e-300, -1e-300, -1e-30], np.float64).astype(dtype)])
        beyond = (o[c] + np.array([KEY_END, KEY_MIN - 1, KEY_END + 5, 4 * KEY_MIN], np.float64) * h
                  + np.array([0.25, 0.25, 0.0, 0.0]) * h).astype(dtype)
        vals = np.concatenate([vals, beyond]).astype(np.float64)
        rows = np.empty((len(vals), 4))
        rows[:, :3] = other
        rows[:, c] = vals
        rows[:, 3] = 0.5
        # the range ends decide by k alone (a float32 value near a UTM-scale end may round to either
        # side): the restatement sorts them; tests/test_voxel_cpu.py pins the exact ends by hand
        K, _, _, bad = quantise(rows[:, :3], rows[:, 3], h, o)
        acc.append(rows[~bad])
        ref.append(rows[bad])
        bad_rows = np.empty((3, 4))
        bad_rows[:, :3] = other
        bad_rows[:, 3] = 0.5
        bad_rows[:, c] = [np.nan, inf, -inf]
        ref.append(bad_rows)
    base = np.empty((4, 4))
    base[:, :3] = (o + 0.25 * h).astype(dtype).astype(np.float64)
    top = np.float64(np.nextafter(np.float32(INT), np.float32(inf)))
    ok_i, bad_i = base.copy(), np.concatenate([base, base[:1]])
    ok_i[:, 3] = [INT, -INT, 0.0, 1.5 / INT]
    bad_i[:, 3] = [top, -top, np.nan, inf, -inf]
    acc.append(ok_i)
    ref.append(bad_i)
    return np.concatenate(acc), np.concatenate(ref)
