"""The surface normals of a voxel cloud restated in NumPy: this project's own definition (include/mcdeskew.h
"surface normals of the voxel cloud"; csrc/normals_core.hpp), which the kernels of csrc/normals.hpp must
reproduce — neighbour counts, kept sets and covariances bit for bit, normals and curvature by the
eigenvector criterion below — and the clouds the tests run it on.

Every line of float64 arithmetic is one IEEE operation on arrays.  The moments are summed over the window's
cells in walk order (dkx, dky, dkz ascending = ascending packed key); a cell that is not a kept neighbour adds
+0.0, which changes no bit of a sum that started at +0.0."""
import math

import numpy as np

import voxel as V

MAX_R = 4
EPS = 2.0 ** -52
# The eigenvector criterion's constant.  Measured on the g++ build of the scalar core over all builder
# clouds below (tests/test_normals_cpu.py prints it): the largest (n^T A n - w0) / (2^-52 |A|_F) is
# MEASURED_C; the bound is four times that, the margin for a device whose sqrt / divide sequence differs.
MEASURED_C = 2.672
C_BOUND = 4 * MEASURED_C


def window_radius(radius, h):
    return int(math.ceil(np.float64(radius) / np.float64(h)))


def estimate(keys, cent, h, radius, max_nn=30):
    """keys (M, 3) int, cent (M, 3) float64 (V.downsample's keys and rows[:, :3]) ->
    dict(counts (M,) int32, cov (M, 6) float64, kept (M, W^3) bool in walk order, R)."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    c = np.ascontiguousarray(np.asarray(cent, np.float64).reshape(-1, 3))
    M = len(keys)
    R = window_radius(radius, h)
    assert 1 <= R <= MAX_R and (max_nn == 0 or 3 <= max_nn <= 64)
    W = 2 * R + 1
    r2 = np.float64(radius) * np.float64(radius)
    packed = V.pack(keys) if M else np.zeros(0, np.int64)
    order = np.argsort(packed)
    sorted_keys = packed[order]
    nbr = np.full((M, W ** 3), -1, np.int64)
    d2 = np.full((M, W ** 3), np.inf)
    ix = 0
    for dx in range(-R, R + 1):
        for dy in range(-R, R + 1):
            for dz in range(-R, R + 1):
                k = keys + np.array([dx, dy, dz])
                ok = ((k >= V.KEY_MIN) & (k < V.KEY_END)).all(axis=1)      # outside: skipped before packing
                want = V.pack(np.where(ok[:, None], k, 0))
                at = np.minimum(np.searchsorted(sorted_keys, want), max(M - 1, 0))
                hit = ok & (sorted_keys[at] == want) if M else ok
                j = order[at[hit]]
                u = c[j] - c[hit]
                xx = u[:, 0] * u[:, 0]
                yy = u[:, 1] * u[:, 1]
                zz = u[:, 2] * u[:, 2]
                xy = xx + yy
                nbr[hit, ix] = j
                d2[hit, ix] = xy + zz
                ix += 1
    kept = d2 <= r2
    if max_nn:
        for i in np.flatnonzero(kept.sum(axis=1) > max_nn):
            cols = np.flatnonzero(kept[i])
            best = cols[np.lexsort((cols, d2[i, cols]))][:max_nn]      # by d2, then by the place in the walk
            kept[i] = False
            kept[i, best] = True
    n = kept.sum(axis=1)
    s = np.zeros((M, 3))
    P = np.zeros((M, 6))
    for ix in range(W ** 3):
        on = kept[:, ix]
        if not on.any():
            continue
        u = np.zeros((M, 3))
        u[on] = c[nbr[on, ix]] - c[on]
        s = s + u
        pr = np.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2],
                       u[:, 2] * u[:, 2]], axis=1)
        pr[~on] = 0.0                     # (-0.0 products of the zero rows)
        P = P + pr
    dn = n.astype(np.float64)[:, None]
    m = s / dn
    E = P / dn
    mm = np.stack([m[:, 0] * m[:, 0], m[:, 0] * m[:, 1], m[:, 0] * m[:, 2], m[:, 1] * m[:, 1], m[:, 1] * m[:, 2],
                   m[:, 2] * m[:, 2]], axis=1)
    return dict(counts=n.astype(np.int32), cov=E - mm, kept=kept, R=R, nbr=nbr)


def of_rows(rows, h, radius, max_nn=30, origin=(0.0, 0.0, 0.0)):
    """The restatement of the voxel filter, then of the normals: (V.downsample(rows), estimate(...))."""
    d = V.downsample(rows, h, origin)
    return d, estimate(d["keys"], d["rows"][:, :3], h, radius, max_nn)


def matrix(cov):
    cov = np.asarray(cov)
    A = np.empty(cov.shape[:-1] + (3, 3))
    for (r, c), k in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}.items():
        A[..., r, c] = A[..., c, r] = cov[..., k]
    return A


def criterion(normals, curvature, cov, counts):
    """The eigenvector criterion on the voxels with three neighbours or more, each figure in units of its
    bound without the constant: -> dict(unit = | |n|^2 - 1 | / 2^-52 (bound 8), rayleigh = (n^T A n - w0) /
    (2^-52 F) (bound c), curv = |curvature - max(w0, 0) / trace| / (2^-52 F / trace) (bound c), gap = w1 - w0,
    F, w).  n^T A n in extended precision, so the figure is the solver's and not this sum's."""
    sel = np.asarray(counts) >= 3
    n = np.asarray(normals, np.float64)[sel]
    A = matrix(np.asarray(cov, np.float64)[sel])
    w = np.linalg.eigvalsh(A) if len(A) else np.zeros((0, 3))
    F = np.sqrt((A * A).sum(axis=(1, 2)))
    nl = n.astype(np.longdouble)
    q = np.einsum("ni,nij,nj->n", nl, A.astype(np.longdouble), nl)
    unit = np.abs((nl * nl).sum(axis=1) - 1).astype(np.float64) / EPS
    tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    pos = (tr > 0) & (F > 0)
    ray = np.zeros(len(A))
    ray[pos] = (q[pos] - w[pos, 0]).astype(np.float64) / (EPS * F[pos])
    curv = np.zeros(len(A))
    curv[pos] = np.abs(np.asarray(curvature)[sel][pos] - np.maximum(w[pos, 0], 0) / tr[pos]) / (EPS * F[pos] / tr[pos])
    return dict(sel=sel, unit=unit, rayleigh=ray, curv=curv, gap=w[:, 1] - w[:, 0], F=F, w=w, trace=tr)


def check_against(est, normals, curvature, counts, cov, viewpoint=None, cent=None, what=""):
    """A build's output against the restatement: counts and covariance bit for bit, normals and curvature by
    the criterion, the sign rule, and (0, 0, 1) / 0 below three neighbours.  -> the criterion's figures"""
    assert np.array_equal(counts, est["counts"]), what
    assert np.array_equal(np.ascontiguousarray(cov).view(np.uint64), np.ascontiguousarray(est["cov"]).view(np.uint64)), what
    few = est["counts"] < 3
    assert (normals[few] == [0.0, 0.0, 1.0]).all() and (curvature[few] == 0.0).all(), what
    k = criterion(normals, curvature, est["cov"], est["counts"])
    if len(k["unit"]):
        assert k["unit"].max() <= 8, (what, k["unit"].max())
        assert k["rayleigh"].max() <= C_BOUND, (what, k["rayleigh"].max())
        assert k["curv"].max() <= C_BOUND, (what, k["curv"].max())
    n = normals[~few]
    if viewpoint is None:
        big = n[np.arange(len(n)), np.abs(n).argmax(axis=1)]       # argmax: the first (lowest) axis of a tie
        assert (big > 0).all(), what
    else:
        w = np.asarray(viewpoint, np.float64) - cent[~few]
        assert ((n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2] >= 0).all(), what
    return k


# ---- the clouds ------------------------------------------------------------------------------------------------
PLANE_NORMAL = np.array([-0.3, 0.2, 1.0]) / np.sqrt(0.3 ** 2 + 0.2 ** 2 + 1.0)


def plane():
    """3 000 seeded points on z = 0.3 x - 0.2 y + 100 with x, y around 1000 (GPS-scale coordinates), the
    reference's own parameters: -> rows, h = 0.05, radius = 0.1; about 1 500 voxels."""
    rng = np.random.default_rng(20251020)
    xy = 1000.0 + rng.uniform(0.0, 1.8, (3000, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 100.0
    return np.column_stack([xy, z, rng.uniform(0.0, 1.0, 3000)]), 0.05, 0.1


def block():
    """8 x 8 x 8 occupied cells, one point at each exact cell centre: -> rows, h = 0.5, radius = 1.0.  An
    interior voxel has 33 neighbours (1 + 6 + 12 + 8 + 6 at 0, 1, sqrt 2, sqrt 3 and 2 cells), of which
    max_nn = 30 keeps three of the six at exactly two cells: ties broken by key."""
    k = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    k = k[np.random.default_rng(8).permutation(len(k))]
    return np.column_stack([(k + 0.5) * 0.5, np.full(len(k), 0.25)]), 0.5, 1.0


ISOLATED_CELLS = np.array([[0, 0, 0], [20, 3, -7], [21, 3, -7], [40, -9, 5], [41, -9, 5], [42, -9, 5]])
ISOLATED_COUNTS = [1, 2, 2, 3, 3, 3]


def isolated():
    """One voxel alone, a pair, and three collinear voxels whose ends are exactly the radius apart, in one
    cloud at exact cell centres: -> rows, h = 0.5, radius = 1.0; counts 1, 2, 2, 3, 3, 3."""
    return np.column_stack([(ISOLATED_CELLS + 0.5) * 0.5, np.full(len(ISOLATED_CELLS), 0.5)]), 0.5, 1.0


def blind_cell(k):
    """The cell whose key a window cell k outside the key range would get if it were packed without the range
    check (the filter's voxel_pack on 32-bit fields: the 22nd bit of an axis spills into the next axis up)."""
    b = [(int(x) - V.KEY_MIN) & 0xFFFFFFFF for x in k]
    key = ((b[0] << 42) | (b[1] << 21) | b[2]) & (2 ** 64 - 1)
    assert key >> 63 == 0
    return [((key >> s) & 0x1FFFFF) + V.KEY_MIN for s in (42, 21, 0)]


def key_ends():
    """Voxels at kx = -2^20 and at ky = 2^20 - 1, each with two true neighbours, and decoys exactly where a
    window key packed without the range check would land: ky = 2^20 of the voxel at kx = 10 is (11, -2^20, kz),
    and that decoy's own ky - 1 is (2047, 2^20 - 1, kz).  -> rows, h = 0.5, radius = 1.0, and the number of
    neighbours each voxel has."""
    lo, hi = V.KEY_MIN, V.KEY_END - 1
    decoy = blind_cell([10, hi + 1, -3])
    cells = np.array([[lo, 5, 5], [lo, 6, 5], [lo, 5, 6],               # the kx end and its neighbours
                      [10, hi, -3], [10, hi - 1, -3], [11, hi, -3],      # the ky end and its neighbours
                      decoy, blind_cell([decoy[0], decoy[1] - 1, decoy[2]])])
    assert cells[6].tolist() == [11, lo, -3] and cells[7].tolist() == [2047, hi, -3]
    rng = np.random.default_rng(21)
    pts = (cells + rng.uniform(0.4, 0.6, cells.shape)) * 0.5
    return np.column_stack([pts, np.full(len(cells), 0.5)]), 0.5, 1.0, [3, 3, 3, 3, 3, 3, 1, 1]


def slab(M, seed, h=0.2):
    """M voxels of one random point each, in distinct random cells of a slab three cells thick that is
    about a quarter occupied: -> rows, h, radius = 2 h."""
    rng = np.random.default_rng(seed)
    side = max(4, int(math.ceil(math.sqrt(M / 0.75))))
    cell = rng.permutation(side * side * 3)[:M]
    k = np.stack([cell // (side * 3) - side // 2, (cell // 3) % side - side // 2, cell % 3 - 1], axis=1)
    pts = (k + rng.uniform(0.05, 0.95, (M, 3))) * h
    return np.column_stack([pts, rng.uniform(0.0, 1.0, M)]), h, 2 * h


def plane_angle_bound(k, h):
    """The angle (rad) between a plane cloud's analytic normal and the returned one, per voxel: the
    criterion bounds the squared sine to the eigenspace of C by C_BOUND 2^-52 F / gap; and C's own
    eigenvector is off the plane's normal by at most |dC| / gap (Davis-Kahan), where the centroids are off
    the plane by at most delta = sqrt(3) (h 2^-32 + 8 ulp(1100)) — the voxel filter's fixed point and the
    float64 rounding of the points and centroids at these coordinates — so |dC| <= 4 delta sqrt(trace)."""
    delta = math.sqrt(3.0) * (h * 2.0 ** -32 + 8 * np.spacing(1100.0))
    return np.sqrt(C_BOUND * EPS * k["F"] / k["gap"]) + 4 * delta * np.sqrt(k["trace"]) / k["gap"]


# ---- the cases, computed once per session and shared (nobody writes into what case() returns) --------------------
CASES = {
    # name: (builder, its arguments, radius in voxels or None for the builder's own, max_nn)
    "plane": (plane, (), None, 30),
    "block": (block, (), None, 30),                 # the cap path, ties broken by key
    "block uncapped": (block, (), None, 0),         # its twin without a cap
    "isolated": (isolated, (), None, 30),
    "key ends": (key_ends, (), None, 30),
    "30 voxels": (slab, (30, 30), None, 30),        # the 64-slot table: chains
    "257 voxels": (slab, (257, 257), None, 30),     # a ragged last workgroup
    "70001 voxels": (slab, (70001, 70001), None, 30),   # more than one wave per SIMD
    "R = 1": (slab, (257, 257), 0.9, 30),
    "R = 4": (slab, (257, 257), 4.0, 30),           # 729 cells; the cap applies to many voxels
    "R = 4 at the fewest": (slab, (257, 257), 4.0, 3),
    "R = 4 at the most": (slab, (257, 257), 4.0, 64),
}
_cache = {}


def case(name, origin=V.ZERO):
    """-> dict(rows, h, origin, radius, max_nn, vox = V.downsample(rows, h, origin), est = estimate(...))"""
    origin = tuple(float(v) for v in origin)
    key = name if origin == V.ZERO else (name, origin)
    if key not in _cache:
        builder, args, rel, max_nn = CASES[name]
        rows, h, radius = builder(*args)[:3]
        if rel is not None:
            radius = rel * h
        d, est = of_rows(rows, h, radius, max_nn, origin)
        _cache[key] = dict(rows=rows, h=h, origin=origin, radius=radius, max_nn=max_nn, vox=d, est=est)
    return _cache[key]


def grid_rows(grid, float32=False):
    """The cloud of every analysis' grid cases: slab(257, 257, h) with the h of V.ORIGIN_GRIDS[grid], where that grid
    has its cloud; float32: the values a batch can hold.  Off the default origin two of its points may share a cell:
    237 to 257 voxels."""
    rows = V.on_grid(slab(257, 257, V.ORIGIN_GRIDS[grid]["h"])[0], grid)
    return V.as_float32(rows) if float32 else rows


def grid_case(grid, rel=2.0, max_nn=30, float32=False):
    """case()'s dict for grid_rows(grid) on the grid's h and origin, at radius = rel h."""
    key = ("grid", grid, rel, max_nn, float32)
    if key not in _cache:
        g = V.ORIGIN_GRIDS[grid]
        rows, h, origin = grid_rows(grid, float32), g["h"], g["origin"]
        d, est = of_rows(rows, h, rel * h, max_nn, origin)
        _cache[key] = dict(rows=rows, h=h, origin=origin, radius=rel * h, max_nn=max_nn, vox=d, est=est)
    return _cache[key]
