"""The registration of a source against a voxel cloud restated in NumPy: this project's own definition
(include/mcdeskew.h "registration against the voxel cloud"; csrc/register_core.hpp), which the kernels of
csrc/register.hpp and the host loop must reproduce bit for bit — the nearest voxel and its squared distance of every
point, the 28 tree sums, every iteration's step, the final pose and the status — and the clouds the tests run it on.

Every line of float64 arithmetic is one IEEE operation, on arrays where it is per point and on Python floats (IEEE
float64, math.sqrt correctly rounded) in the 6 x 6 solve and the pose update.  The cloud's normals and their
neighbour counts are an input: the bits of VoxelCloud.normals(normals_radius, max_nn), or of the host core in the
CPU tests (tests/normals.py holds those to its criterion).

The cases.  CASES: all on the default origin, where the o terms of RegSkip's cell faces o + k h are zero.  grid_case:
tests/normals.py's 257-point slab and 1281 scattered source points on the grids of tests/voxel.py ORIGIN_GRIDS — utm
(the cloud and the source at a UTM-scale origin: o dominates o + k h and the skip's slack is at its largest),
fractional (no axis of o is a multiple of h: the cell faces are not the default grid's), far keys (the cloud near zero,
the origin far: keys near (825 000, -500 000, 250 000) and o + k h cancelling) and the same on h = 7.3 — at W = 1, 2
and 4, from the identity and from NEARBY.  nearest() here walks every cell; the core leaves cells out, so these cases
are the check that the skip changes no output.  At utm the step itself is ill-conditioned (the normal equations are
taken about the world's origin, cond(A) about 1e26): the first step throws the source off the cloud and the second
iteration ends with too_few_pairs; every bit of that is still the definition's.  radius_edges: on each grid 64 queries
at the smallest max_distance that reaches their nearest centroid, and at the float64 below."""
import math

import numpy as np

import normals as N
import planes as P
import voxel as V

STATUS = ("converged", "max_iterations", "too_few_pairs", "singular")
SUMS = 28
MIN_PAIRS = 6


def move(T, p):
    """q = R p + t for p (n, 3), T (4, 4)."""
    T = np.asarray(T, np.float64)
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((T[c, 0] * p[:, 0] + T[c, 1] * p[:, 1]) + T[c, 2] * p[:, 2]) + T[c, 3] for c in range(3)], axis=1)


def nearest(keys, cent, h, origin, q, max_distance):
    """keys (M, 3), cent (M, 3) of the cloud; q (n, 3) moved points -> ids (n,) int32, dist2 (n,) float64."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    c = np.ascontiguousarray(np.asarray(cent, np.float64).reshape(-1, 3))
    q = np.asarray(q, np.float64).reshape(-1, 3)
    n, M = len(q), len(keys)
    ids = np.full(n, -1, np.int32)
    best = np.full(n, np.inf)
    if M == 0:
        return ids, best
    W = max(1, N.window_radius(max_distance, h))
    assert W <= N.MAX_R
    r2 = np.float64(max_distance) * np.float64(max_distance)
    kq, _, _, bad = V.quantise(q, np.zeros(n), h, origin)
    packed = V.pack(keys)
    order = np.argsort(packed)
    sorted_keys = packed[order]
    for dx in range(-W, W + 1):
        for dy in range(-W, W + 1):
            for dz in range(-W, W + 1):
                k = kq + np.array([dx, dy, dz])
                ok = ~bad & ((k >= V.KEY_MIN) & (k < V.KEY_END)).all(axis=1)
                want = V.pack(np.where(ok[:, None], k, 0))
                at = np.minimum(np.searchsorted(sorted_keys, want), M - 1)
                hit = ok & (sorted_keys[at] == want)
                j = order[at[hit]]
                u = c[j] - q[hit]
                xx = u[:, 0] * u[:, 0]
                yy = u[:, 1] * u[:, 1]
                zz = u[:, 2] * u[:, 2]
                xy = xx + yy
                d2 = xy + zz
                rows = np.flatnonzero(hit)
                better = (d2 <= r2) & (d2 < best[rows])          # a tie stays with the cell walked first
                ids[rows[better]] = j[better]
                best[rows[better]] = d2[better]
    return ids, best


def leaves(q, c, n, pair):
    """The 28 leaves of every point: q (n, 3), its pair's centroid c and normal n (rows without a pair: anything)."""
    with np.errstate(all="ignore"):
        d = q - c
        r = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        a = np.stack([q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2],
                      q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0]], axis=1)
        J = np.concatenate([a, n], axis=1)
        cols = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r]
    out = np.stack(cols, axis=1)
    out[~pair] = 0.0
    return out


def tree_sums(leaf):
    return np.array([P.tree(leaf[:, k]) for k in range(SUMS)])


def solve(s):
    """A x = -b of the 28 sums by Cholesky -> x (6,) or None when a pivot is not finite or not > 0."""
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(s[at])
            at += 1
    b = [float(v) for v in s[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            acc = A[i][j]
            for k in range(j):
                p = L[i][k] * L[j][k]
                acc = acc - p
            if j == i:
                if not (math.isfinite(acc) and acc > 0.0):
                    return None
                L[i][i] = math.sqrt(acc)
            else:
                L[i][j] = acc / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        acc = -b[i]
        for k in range(i):
            p = L[i][k] * y[k]
            acc = acc - p
        y[i] = acc / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        acc = y[i]
        for k in range(i + 1, 6):
            p = L[k][i] * x[k]
            acc = acc - p
        x[i] = acc / L[i][i]
    return np.array(x)


def rotation(w):
    """The rotation of the unit quaternion (1, w / 2) / |(1, w / 2)|."""
    hx, hy, hz = 0.5 * float(w[0]), 0.5 * float(w[1]), 0.5 * float(w[2])
    n = math.sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    qw, qx, qy, qz = 1.0 / n, hx / n, hy / n, hz / n
    xx, yy, zz = qx * qx, qy * qy, qz * qz
    xy, xz, yz = qx * qy, qx * qz, qy * qz
    wx, wy, wz = qw * qx, qw * qy, qw * qz
    return np.array([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                     [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                     [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]])


def update(T, x):
    """R <- dR R, t <- dR t + v."""
    D = rotation(x[:3]).tolist()
    R = T[:3, :3].tolist()
    t = T[:3, 3].tolist()
    out = np.eye(4)
    for r in range(3):
        for c in range(3):
            out[r, c] = (D[r][0] * R[0][c] + D[r][1] * R[1][c]) + D[r][2] * R[2][c]
        out[r, 3] = ((D[r][0] * t[0] + D[r][1] * t[1]) + D[r][2] * t[2]) + float(x[3 + r])
    return out


def small(x, tol_rotation, tol_translation):
    x = [float(v) for v in x]
    ww = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    vv = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
    return ww <= float(tol_rotation) * float(tol_rotation) and vv <= float(tol_translation) * float(tol_translation)


def register(cloud, src, max_distance, init=None, max_iterations=30, tol_rotation=1e-6, tol_translation=1e-6):
    """cloud: dict(keys (M, 3), cent (M, 3), h, origin, normals (M, 3), counts (M,)); src (n, 3) float64 ->
    dict(transformation, fitness, inlier_rmse, pairs, iterations, status, history (iterations, 8), and per iteration
    ids, dist2 and sums)."""
    src = np.ascontiguousarray(np.asarray(src, np.float64)[:, :3])
    n = len(src)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    nrm = np.asarray(cloud["normals"], np.float64).reshape(-1, 3)
    counts = np.asarray(cloud["counts"]).reshape(-1)
    cent = np.asarray(cloud["cent"], np.float64).reshape(-1, 3)
    history, all_ids, all_d2, all_sums = [], [], [], []
    status = None
    pairs = 0
    for _ in range(max_iterations):
        q = move(T, src)
        ids, d2 = nearest(cloud["keys"], cent, cloud["h"], cloud["origin"], q, max_distance)
        at = np.maximum(ids, 0)
        pair = (ids >= 0) & (counts[at] >= 3) if len(counts) else np.zeros(n, bool)
        leaf = leaves(q, cent[at], nrm[at], pair) if len(counts) else np.zeros((n, SUMS))
        s = tree_sums(leaf)
        pairs = int(pair.sum())
        row = np.zeros(8)
        row[0], row[1] = pairs, s[27]
        all_ids.append(ids)
        all_d2.append(d2)
        all_sums.append(s)
        history.append(row)
        if pairs < MIN_PAIRS:
            status = "too_few_pairs"
            break
        x = solve(s)
        if x is None:
            status = "singular"
            break
        row[2:] = x
        T = update(T, x)
        if small(x, tol_rotation, tol_translation):
            status = "converged"
            break
    if status is None:
        status = "max_iterations"
    history = np.array(history)
    rmse = math.sqrt(float(history[-1, 1]) / pairs) if pairs else 0.0
    return dict(transformation=T, fitness=pairs / n, inlier_rmse=rmse, pairs=pairs, iterations=len(history), status=status,
                history=history, ids=all_ids, dist2=all_d2, sums=all_sums)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def equal(got, want):
    """A VoxelRegistration (or the host harness's dict) against the restatement: every field bit for bit."""
    g = got._asdict() if hasattr(got, "_asdict") else got
    return (g["status"] == want["status"] and g["iterations"] == want["iterations"] and g["pairs"] == want["pairs"]
            and np.array_equal(bits(g["history"]), bits(want["history"]))
            and np.array_equal(bits(g["transformation"]), bits(want["transformation"]))
            and bits(g["fitness"]) == bits(want["fitness"]) and bits(g["inlier_rmse"]) == bits(want["inlier_rmse"]))


# ---- the clouds ------------------------------------------------------------------------------------------------
H = 0.25


def pose(rx, ry, rz, t):
    """A rotation about x, then y, then z by the three angles, and a translation, as a 4 x 4."""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


KNOWN = pose(0.02, -0.015, 0.0175, [0.04, -0.03, 0.033])          # |w| = 0.03 rad, |t| = 0.06 m


def corner_rows(h=H, side=16, seed=7):
    """Three mutually perpendicular patches of side x side voxels, two points in every voxel: z = h / 2 over x, y in
    [1, 1 + side h), x = h / 2 over y, z there, y = h / 2 over x, z there.  The offset h / 2 is exact in the filter's
    fixed point, so every centroid lies exactly on its plane; the patches are 0.875 m from the axes they would meet
    on, further than the normals' radius of 2 h, so every normal is an axis exactly.  -> rows (n, 4)"""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)
    ij = np.repeat(ij, 2, axis=0)
    uv = 1.0 + (ij + rng.integers(1, 255, ij.shape) / 256.0) * h
    flat = np.full(len(uv), h / 2)
    pts = np.concatenate([np.column_stack([uv, flat]), np.column_stack([flat, uv]), np.column_stack([uv[:, 0], flat, uv[:, 1]])])
    pts = pts[rng.permutation(len(pts))]
    return np.column_stack([pts, np.full(len(pts), 0.5)])


def corner_source(n, seed, h=H, side=16, planes=(0, 1, 2)):
    """n points lying exactly on the patches of corner_rows (the planes named), half a metre inside their rims."""
    rng = np.random.default_rng(seed)
    uv = 1.5 + rng.integers(0, int((side * h - 1.0) * 4096), (n, 2)) / 4096.0
    flat = np.full(n, h / 2)
    which = np.asarray(planes)[rng.integers(0, len(planes), n)]
    on = [np.column_stack([uv, flat]), np.column_stack([flat, uv]), np.column_stack([uv[:, 0], flat, uv[:, 1]])]
    return np.where((which == 0)[:, None], on[0], np.where((which == 1)[:, None], on[1], on[2]))


def moved_back(points, T):
    """The source that T carries onto `points` (float64 rounding apart): R^T (q - t)."""
    return (points - T[:3, 3]) @ T[:3, :3]


def slab_source(n, seed, h=0.2):
    """n points scattered through and around N.slab's three-cell layer: near, between and away from its voxels."""
    rng = np.random.default_rng(seed)
    side = max(4, int(math.ceil(math.sqrt(257 / 0.75))))
    lo = np.array([-side // 2 - 1, -side // 2 - 1, -3]) * h
    hi = np.array([side - side // 2 + 1, side - side // 2 + 1, 4]) * h
    return rng.uniform(lo, hi, (n, 3))


_cache = {}


def corner(origin=V.ZERO):
    """-> dict(rows, h, origin, vox = V.downsample(rows, h, origin), keys, cent); nobody writes into it"""
    origin = tuple(float(v) for v in origin)
    key = ("corner", origin)
    if key not in _cache:
        rows = corner_rows()
        d = V.downsample(rows, H, origin)
        _cache[key] = dict(rows=rows, h=H, origin=origin, vox=d, keys=d["keys"], cent=np.ascontiguousarray(d["rows"][:, :3]))
    return _cache[key]


def with_normals(cloud, normals, counts):
    """The cloud with the normals a build returned (the restatement's input)."""
    return dict(cloud, normals=np.asarray(normals, np.float64)[:, :3], counts=np.asarray(counts))


def expect(key, cloud, src, max_distance, **kw):
    """The restatement of a case, computed once per session under `key` and shared (nobody writes into it)."""
    if key not in _cache:
        _cache[key] = register(cloud, src, max_distance, **kw)
    return _cache[key]


# ---- the cases: name -> dict(rows, h, src, max_distance, radius, max_nn, init, max_iterations) -------------------
def _case(rows, h, src, max_distance, radius=None, max_nn=30, init=None, max_iterations=3):
    return dict(rows=np.asarray(rows, np.float64), h=h, src=np.ascontiguousarray(src, dtype=np.float64), max_distance=max_distance,
                radius=2 * h if radius is None else radius, max_nn=max_nn, init=init, max_iterations=max_iterations)


SIZES = (1, 255, 256, 257, 1281)      # the tree's block edge and padded partials (65 537, a third level: GPU only)
NEARBY = pose(0.01, 0.02, -0.015, [0.03, -0.02, 0.05])


def known_answer(n=3000, max_iterations=30, init=None, max_distance=2 * H):
    """The corner cloud, n source points on its planes moved back by KNOWN: the registration recovers KNOWN."""
    return _case(corner_rows(), H, moved_back(corner_source(n, n), KNOWN), max_distance, init=init, max_iterations=max_iterations)


def slab_case(n, rel=2.0, init=None, h=0.2):
    """n scattered points against tests/normals.py's slab of 257 voxels, max_distance = rel h."""
    return _case(N.slab(257, 257, h)[0], h, slab_source(n, n, h), rel * h, init=init)


def centres(cells, h):
    """One point at the exact centre of every cell, in the order given: -> rows"""
    return np.column_stack([(np.asarray(cells, np.float64) + 0.5) * h, np.full(len(cells), 0.5)])


TIE_CELLS = [[1, 0, 0], [0, 0, 0], [4, 4, 1], [4, 4, 0], [-7, -3, -2], [-7, -4, -2]]
TIE_WINNERS = [1, 3, 5]               # the lower cell key of each pair, here always the higher voxel id


def tie():
    """Three pairs of voxels at exact cell centres of h = 0.5, adjacent along x, z and y (the last at negative keys),
    the voxel of the higher key first in the cloud; each query is exactly midway, on dyadic coordinates, so both d2
    are 0.0625 exactly: the lower cell key wins, whatever cell the query itself falls in."""
    h = 0.5
    c = (np.asarray(TIE_CELLS, np.float64) + 0.5) * h
    src = np.stack([(c[0] + c[1]) / 2, (c[2] + c[3]) / 2, (c[4] + c[5]) / 2])
    return _case(centres(TIE_CELLS, h), h, src, 1.0, max_iterations=1)


EDGE_D = 0.75


def radius_edge(under=False):
    """A voxel at the exact centre of cell (0, 0, 0) of h = 0.5 and queries exactly 0.75 = 1.5 h from it along z, y and
    x: taken at max_distance = 0.75 (d2 = 0.5625 = r2), not taken at the float64 below."""
    h = 0.5
    c = np.array([0.25, 0.25, 0.25])
    src = np.stack([c + [0, 0, EDGE_D], c - [0, EDGE_D, 0], c + [EDGE_D, 0, 0], c + [0.125, 0, 0]])
    d = float(np.nextafter(np.float64(EDGE_D), 0.0)) if under else EDGE_D
    return _case(centres([[0, 0, 0]], h), h, src, d, max_iterations=1)


def window_edges(rel):
    """tests/normals.py's cloud at both ends of the key range, with its decoys where a key packed without the range
    check would land.  Queries: beside every voxel (their windows cross the range's ends), in empty cells next to
    occupied ones (negative keys among them), one NaN, one infinite, and two beyond +-2^20 h: those four get -1 and
    inf and leave the rest alone."""
    rows, h = N.key_ends()[:2]
    rng = np.random.default_rng(5)
    at = rows[:, :3]
    big = float(V.KEY_END) * h
    src = np.concatenate([at + rng.uniform(-0.2, 0.2, at.shape) * h, at + [0.0, 0.0, h], at - [0.0, h, 0.0],
                          [[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [big + 1.0, 1.0, 1.0], [1.0, 1.0, -big - 1.0]]])
    return _case(rows, h, src, rel * h, max_iterations=1)


def few_neighbours(n_pairs=5):
    """tests/normals.py's isolated voxels (neighbour counts 1, 2, 2, 3, 3, 3 at the radius of 2 h): two source points
    beside every voxel with fewer than three neighbours, which find it and are dropped, and n_pairs beside the three
    that have them."""
    rows, h, radius = N.isolated()
    rng = np.random.default_rng(6)
    at = rows[:, :3]
    near = np.concatenate([np.repeat(at[:3], 2, axis=0), at[3 + np.arange(n_pairs) % 3]])
    return _case(rows, h, near + rng.uniform(-0.1, 0.1, near.shape) * h, h, radius=radius, max_iterations=2)


def one_plane(n=300):
    """The corner cloud and a source on its z plane alone: J's third, fourth and fifth components are exactly zero, so
    the third pivot is exactly zero."""
    return _case(corner_rows(), H, corner_source(n, n, planes=(0,)), 2 * H, init=NEARBY_FLAT, max_iterations=5)


NEARBY_FLAT = pose(0.0, 0.0, 0.01, [0.02, -0.01, 0.0])      # keeps the z plane on itself

CASES = {
    "known answer": (known_answer, ()),
    "known answer from the answer": (known_answer, (3000, 30, KNOWN)),
    "known answer, one iteration": (known_answer, (3000, 1)),
    **{f"slab {n}": (slab_case, (n,)) for n in SIZES},
    "slab 257, W = 1": (slab_case, (257, 0.9)),
    "slab 257, W = 4": (slab_case, (257, 4.0, NEARBY)),
    "slab 1281 from a pose": (slab_case, (1281, 2.0, NEARBY)),
    "tie": (tie, ()),
    "radius edge": (radius_edge, ()),
    "radius edge, the float64 below": (radius_edge, (True,)),
    "window edges, W = 1": (window_edges, (1.0,)),
    "window edges, W = 4": (window_edges, (4.0,)),
    "few neighbours": (few_neighbours, ()),
    "six pairs": (few_neighbours, (6,)),
    "one plane": (one_plane, ()),
}


def _voxelised(c, origin):
    d = V.downsample(c["rows"], c["h"], origin)
    c.update(vox=d, keys=d["keys"], cent=np.ascontiguousarray(d["rows"][:, :3]), origin=origin)
    return c


def case(name, origin=V.ZERO):
    """-> the case's dict with vox = V.downsample(rows, h, origin), keys and cent; nobody writes into it"""
    origin = tuple(float(v) for v in origin)
    k = ("case", name) if origin == V.ZERO else ("case", name, origin)
    if k not in _cache:
        builder, args = CASES[name]
        _cache[k] = _voxelised(builder(*args), origin)
    return _cache[k]


def expect_case(name, normals, counts, c=None):
    """The restatement of a case on the normals a build returned (cached per case and normals); c: a grid case's
    dict, with `name` the key it is kept under."""
    c = case(name) if c is None else c
    given = (np.ascontiguousarray(normals, np.float64)[:, :3].tobytes(), np.ascontiguousarray(counts, np.int32).tobytes())
    return expect(("expect", name, hash(given)), with_normals(c, normals, counts), c["src"], c["max_distance"], init=c["init"],
                  max_iterations=c["max_iterations"])


# ---- the grids off the default origin (V.ORIGIN_GRIDS) ----------------------------------------------------------
GRID_RUNS = tuple((rel, init) for rel in (0.9, 2.0, 4.0) for init in ("identity", "nearby"))       # W = 1, 2, 4


def grid_case(grid, rel=2.0, init="identity", float32=False):
    """N.grid_rows(grid) on the grid's h and origin, and slab_source(1281, 1281, h) where that grid has its cloud, at
    max_distance = rel h for three iterations.  init "nearby": from the pose NEARBY; where the grid moves its cloud
    the source is moved back by NEARBY first (a rotation of coordinates of millions of metres would carry it
    kilometres off the cloud), so that NEARBY brings it onto the cloud again.  float32: cloud and source hold the
    values a batch can hold."""
    k = ("grid", grid, rel, init, float32)
    if k not in _cache:
        g = V.ORIGIN_GRIDS[grid]
        src = V.on_grid(slab_source(1281, 1281, g["h"]), grid)
        if init == "nearby" and g["moved"]:
            src = moved_back(src, NEARBY)
        if float32:
            src = V.as_float32(src)
        c = _case(N.grid_rows(grid, float32), g["h"], src, rel * g["h"], init=NEARBY if init == "nearby" else None)
        _cache[k] = _voxelised(c, g["origin"])
    return _cache[k]


def grid_expect(grid, rel, init, normals, counts, float32=False):
    return expect_case(("grid", grid, rel, init, float32), normals, counts, grid_case(grid, rel, init, float32))


def d2_of(cent, q):
    """|c - q|^2 of every centroid in the definition's op order: (xx + yy) + zz of u = c - q."""
    u = cent - q
    return (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]


def reach(d2):
    """The smallest float64 md with md * md >= d2."""
    d2 = np.float64(d2)
    md = np.sqrt(d2)
    while md * md >= d2:
        md = np.nextafter(md, 0.0)
    while md * md < d2:
        md = np.nextafter(md, np.inf)
    return float(md)


EDGE_QUERIES = 64


def radius_edges(grid):
    """The radius edge on a grid's cloud: EDGE_QUERIES seeded queries, each in a random direction at 0.3 h to 3.5 h from
    a randomly chosen centroid (so the nearest centroid is at most 3.5 h away and the window at most four cells).  For
    each the brute-force nearest centroid's d2 in the definition's op order, `at` = the smallest float64 whose square
    reaches it, `under` = the float64 below, and the restatement's nearest at both: -> list of dict(q (1, 3), at,
    under, want_at = (ids, d2), want_under).  At `at` the brute-force nearest is within reach; at `under` it is not."""
    k = ("edges", grid)
    if k not in _cache:
        c = grid_case(grid)
        h, cent = c["h"], c["cent"]
        rng = np.random.default_rng(64)
        out = []
        for _ in range(EDGE_QUERIES):
            d = rng.normal(size=3)
            q = (cent[rng.integers(len(cent))] + d / np.linalg.norm(d) * rng.uniform(0.3, 3.5) * h)[None, :]
            at = reach(d2_of(cent, q[0]).min())
            under = float(np.nextafter(at, 0.0))
            out.append(dict(q=q, at=at, under=under, want_at=nearest(c["keys"], cent, h, c["origin"], q, at),
                            want_under=nearest(c["keys"], cent, h, c["origin"], q, under)))
        _cache[k] = out
    return _cache[k]
