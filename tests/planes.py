"""The plane segmentation of a voxel cloud restated in NumPy: this project's own definition (include/mcdeskew.h
"plane segmentation of the voxel cloud"; csrc/plane_core.hpp), which the kernels of csrc/plane.hpp must reproduce —
scores, winner, samples, masks, tree sums, the unrefined model and the refit's covariance bit for bit, the refit's
normal by the eigenvector criterion of tests/normals.py — and the clouds the tests run it on.

Every line of float64 arithmetic is one IEEE operation on arrays; the sampler is uint64 arithmetic that wraps, its
mulhi64 goes through Python ints; the refit's normal is np.linalg.eigh's.

The clouds.  CASES: small clouds for the definition's decisions.  LARGE: slabs at the sizes where the code changes
shape — 32 769 voxels, the smallest cloud whose 65 536 leaves give the refit a second tree level on the device (one
workgroup, half the first level padding); 65 537, whose 131 072 leaves give two second-level workgroups and two
partials for the host, and the first size at which compact()'s scan of the workgroup counts has a 257th count;
2048 * 1024 + 1025 = 2 098 177, where the score kernel's 2 048 workgroups walk 2 050 tiles, one a full second tile and
one a ragged tile of one voxel (K = 8: the restatement is the slow side, and its winner leads by more than a tile).
grid_case: slab(257) on the grids of tests/voxel.py ORIGIN_GRIDS, off the default origin."""
import math

import numpy as np

import normals as N
import voxel as V

GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
MAX_ITERATIONS = 2 ** 20
U = np.uint64


def mix(z):
    """splitmix64's finaliser on a uint64 array (wrapping)."""
    z = np.asarray(z, U)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def mulhi64(r, n):
    return np.array([(int(x) * int(n)) >> 64 for x in r], np.int64)


def sample(seed, K, n):
    """-> (K, 3) places in ids: distinct by construction."""
    assert n >= 3 and 0 <= seed <= MASK64
    with np.errstate(over="ignore"):
        k3 = U(3) * np.arange(K, dtype=U)
        r = [mix(U(seed) + U(GOLDEN) * (k3 + U(j + 1))) for j in range(3)]
    a = mulhi64(r[0], n)
    b = mulhi64(r[1], n - 1)
    b = b + (b >= a)
    c = mulhi64(r[2], n - 2)
    c = c + (c >= np.minimum(a, b))
    c = c + (c >= np.maximum(a, b))
    return np.stack([a, b, c], axis=1)


def hypotheses(p0, p1, p2, t):
    """(K, 3) samples -> dict(n (K, 3), l2, d, tau, valid)"""
    t = np.float64(t)
    with np.errstate(all="ignore"):
        e1 = p1 - p0
        e2 = p2 - p0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        l2 = (nx * nx + ny * ny) + nz * nz
        d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
        tau = (t * t) * l2
    valid = (l2 > 0) & np.isfinite(l2) & np.isfinite(d) & np.isfinite(tau)
    return dict(n=np.stack([nx, ny, nz], axis=1), l2=l2, d=d, tau=tau, valid=valid)


def offsets(n, d, c):
    """s of every centroid c (m, 3) under one plane."""
    return ((n[0] * c[:, 0] + n[1] * c[:, 1]) + n[2] * c[:, 2]) + d


def tree(a):
    """The balanced adjacent-pair tree over the leaves padded with +0.0 to the power of two >= max(len, 256)."""
    L = 256
    while L < len(a):
        L *= 2
    a = np.concatenate([np.asarray(a, np.float64), np.zeros(L - len(a))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def plane_leaves_of(M):
    """The tree's leaves for M voxels."""
    L = 256
    while L < M:
        L *= 2
    return L


def signed(model):
    """The sign rule: negated when the component of the normal of largest magnitude is negative (lowest axis on a tie)."""
    return -model if model[int(np.abs(model[:3]).argmax())] < 0 else model


def moments(cent, inliers, p0):
    """The nine tree sums s[3], P[6] of the inliers about p0, over all voxel ids."""
    u = np.where(inliers[:, None], cent - p0, 0.0)
    pr = np.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2],
                   u[:, 2] * u[:, 2]], axis=1)
    pr[~inliers] = 0.0                # (-0.0 products of the zero rows)
    return np.array([tree(u[:, c]) for c in range(3)] + [tree(pr[:, c]) for c in range(6)])


def covariance(sums, n_in):
    dn = np.float64(n_in)
    m = sums[:3] / dn
    E = sums[3:] / dn
    mm = np.array([m[0] * m[0], m[0] * m[1], m[0] * m[2], m[1] * m[1], m[1] * m[2], m[2] * m[2]])
    return m, E - mm


def plane_d(nrm, q):
    return -((nrm[0] * q[0] + nrm[1] * q[1]) + nrm[2] * q[2])


def ransac(cent, t, K, seed, refine=True, among=None):
    """cent (M, 3) float64 by voxel id -> dict(model (4,), inliers (M,) bool, n_inliers, score, iteration, samples
    (3,) int32, covariance (6,) or None, refined, scores (K,) int64, valid (K,), sums (9,) or None, hyp_inliers)."""
    cent = np.ascontiguousarray(np.asarray(cent, np.float64).reshape(-1, 3))
    M = len(cent)
    t = np.float64(t)
    assert 1 <= K <= MAX_ITERATIONS
    cand = np.ones(M, bool) if among is None else np.asarray(among, bool)
    ids = np.flatnonzero(cand)
    n = len(ids)
    if n < 3:
        raise ValueError("fewer than three candidates")
    at = ids[sample(seed, K, n)]
    h = hypotheses(cent[at[:, 0]], cent[at[:, 1]], cent[at[:, 2]], t)
    c = cent[ids]
    scores = np.zeros(K, np.int64)
    for k in np.flatnonzero(h["valid"]):
        s = offsets(h["n"][k], h["d"][k], c)
        scores[k] = np.count_nonzero(s * s <= h["tau"][k])
    out = dict(scores=scores, valid=h["valid"], sums=None)
    k = int(np.argmax(scores))                       # argmax: the first (lowest) k of a tie
    if scores[k] < 3:
        out.update(model=np.zeros(4), inliers=np.zeros(M, bool), n_inliers=0, score=0, iteration=-1,
                   samples=np.full(3, -1, np.int32), covariance=None, refined=False, hyp_inliers=np.zeros(M, bool))
        return out
    nk, p0 = h["n"][k], cent[at[k, 0]]
    s = offsets(nk, h["d"][k], cent)
    inl = cand & (s * s <= h["tau"][k])
    assert inl.sum() == scores[k]
    out.update(score=int(scores[k]), iteration=k, samples=at[k].astype(np.int32), hyp_inliers=inl)
    if not refine:
        l = np.sqrt(h["l2"][k])
        nh = nk / l
        model = signed(np.array([nh[0], nh[1], nh[2], plane_d(nh, p0)]))
        out.update(model=model, inliers=inl, n_inliers=int(inl.sum()), covariance=None, refined=False)
        return out
    sums = moments(cent, inl, p0)
    m, cov = covariance(sums, scores[k])
    w, vec = np.linalg.eigh(N.matrix(cov))
    nh = vec[:, 0]
    nh = signed(np.append(nh, 0.0))[:3]
    q = p0 + m
    dh = plane_d(nh, q)
    s = offsets(nh, dh, cent)
    rin = cand & (np.abs(s) <= t)
    out.update(model=np.array([nh[0], nh[1], nh[2], dh]), inliers=rin, n_inliers=int(rin.sum()), covariance=cov, refined=True,
               sums=sums, offsets=s, eigenvalues=w)
    return out


def angle_bound(cov):
    """The angle (rad) the refit's normal may differ from eigh's by: the criterion bounds the squared sine to the
    eigenspace of C by C_BOUND 2^-52 F / gap (tests/normals.py); twice, for the two solvers."""
    A = N.matrix(cov)
    w = np.linalg.eigvalsh(A)
    F = math.sqrt(float((A * A).sum()))
    return 2 * math.sqrt(N.C_BOUND * N.EPS * F / (w[1] - w[0])), F, w[1] - w[0]


def check_refit(model, cov, want, t):
    """A refined model against the restatement's: the covariance bit for bit, the normal by the criterion, unit
    length, the sign rule, and d^ recomputed from the returned normal bit for bit."""
    model = np.asarray(model, np.float64)
    assert np.array_equal(np.asarray(cov, np.float64).view(np.uint64), want["covariance"].view(np.uint64))
    k = N.criterion(model[None, :3], np.zeros(1), want["covariance"][None], np.array([3]))
    assert k["unit"][0] <= 8 and k["rayleigh"][0] <= N.C_BOUND, (k["unit"], k["rayleigh"])
    assert model[int(np.abs(model[:3]).argmax())] > 0
    p0 = want["cent"][want["samples"][0]]
    q = p0 + want["sums"][:3] / np.float64(want["score"])
    assert np.float64(plane_d(model[:3], q)).view(np.uint64) == model[3:].view(np.uint64)[0]
    bound = angle_bound(want["covariance"])[0]
    assert np.linalg.norm(np.cross(model[:3], want["model"][:3])) <= bound, (model, want["model"], bound)


# ---- the clouds ------------------------------------------------------------------------------------------------
def cells(rng, count, side):
    """count distinct (ix, iy) of a side x side grid around the origin."""
    c = rng.permutation(side * side)[:count]
    return np.stack([c // side - side // 2, c % side - side // 2], axis=1)


def slab(M, seed=None, h=0.25, extent=64.0):
    """M voxels of one point each: ceil(0.7 M) on the tilted plane z = 0.3 x - 0.2 y + 1 with a residual of at most
    0.55 t along z (less across the plane), the others 3 t to 10 t above or below it along z (at least 2.8 t across);
    every point in a cell (ix, iy) of its own, so in a voxel of its own on the default grid: -> rows, h, t = h.  The
    cloud is at most `extent` metres wide (what tests/test_planes_cpu.py's bounds on the SLABS assume is 64)."""
    rng = np.random.default_rng(M if seed is None else seed)
    t = h
    side = max(4, int(math.ceil(math.sqrt(2.0 * M))))
    assert side * h <= extent
    n_in = int(math.ceil(0.7 * M))
    xy = (cells(rng, M, side) + rng.uniform(0.2, 0.8, (M, 2))) * h
    off = np.concatenate([rng.uniform(-0.55, 0.55, n_in) * t,
                          rng.uniform(3.0, 10.0, M - n_in) * t * rng.choice([-1.0, 1.0], M - n_in)])
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 1.0 + off
    order = rng.permutation(M)
    return np.column_stack([xy, z, rng.uniform(0.0, 1.0, M)])[order], h, t


SLAB_NORMAL = np.array([-0.3, 0.2, 1.0]) / math.sqrt(0.3 ** 2 + 0.2 ** 2 + 1.0)


def two_planes(h=0.25):
    """40 voxels on z = 1/8 and 40 on z = 5 + 1/8, the same (x, y) in both, at multiples of 2^-8: every pure
    hypothesis holds exactly its plane's 40 voxels, so the winner is decided by the lowest k: -> rows, h, t = 1/64."""
    rng = np.random.default_rng(40)
    xy = (cells(rng, 40, 8) * 64 + rng.integers(8, 56, (40, 2))) / 256.0
    low = np.column_stack([xy, np.full(40, 0.125)])
    pts = np.concatenate([low, low + [0.0, 0.0, 5.0]])[rng.permutation(80)]
    return np.column_stack([pts, np.full(80, 0.5)]), h, 1.0 / 64


def collinear(h=0.25):
    """20 voxels on one line along x, y and z the same in all: every cross product is zero: -> rows, h, t = h."""
    x = (np.random.default_rng(20).permutation(20) + 0.5) * h
    return np.column_stack([x, np.full(20, 0.125), np.full(20, 0.375), np.full(20, 0.5)]), h, h


EDGE_T = 2.0 ** -4


def dyadic_edge(h=0.25):
    """24 voxels on z = 0 in a ring of half a metre to a metre around (1, 1), at multiples of 2^-8 (every product of
    a hypothesis in the plane and of its tests is exact), in the ring's middle voxel 24 at z = t = 2^-4 exactly and
    voxel 25 at z = t + h 2^-32, the next centroid the filter can hold, and two far voxels: -> rows, h, t.  A tilted
    plane through a middle voxel leaves half the ring out, so a hypothesis in the plane wins.  (A point at the next
    float64 above t does not survive the filter's 2^-32 h fixed point; the second run, at the float64 below t, puts
    voxel 24 exactly at the next float64 above its threshold instead.)"""
    rng = np.random.default_rng(24)
    ij = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 2)
    r = np.linalg.norm((ij + 0.5) * h - 1.0, axis=1)
    ring = ij[(r >= 0.5) & (r <= 1.0)]
    ring = ring[rng.permutation(len(ring))[:24]]
    ij = np.concatenate([ring, [[3, 3], [4, 4], [0, 0], [7, 7]]])
    xy = (ij * 64 + rng.integers(8, 56, (28, 2))) / 256.0
    z = np.concatenate([np.zeros(24), [EDGE_T, EDGE_T + h * 2.0 ** -32, 1.0, -1.0]])
    return np.column_stack([xy, z, np.full(28, 0.5)]), h, EDGE_T


def ground_wall(h=0.25):
    """300 voxels of a ground z ~ 0, 150 of a wall x ~ 6 above it and 50 scattered: -> rows, h, t = h / 2."""
    rng = np.random.default_rng(300)
    t = h / 2
    g = np.column_stack([(cells(rng, 300, 40) + rng.uniform(0.2, 0.8, (300, 2))) * h, rng.uniform(-0.5, 0.5, 300) * t])
    yz = (cells(rng, 150, 20) + [0, 14] + rng.uniform(0.2, 0.8, (150, 2))) * h          # z from a metre up
    w = np.column_stack([6.0 + rng.uniform(-0.5, 0.5, 150) * t, yz])
    s = np.column_stack([rng.uniform(-4.0, 4.0, (50, 2)), rng.uniform(8.0, 12.0, 50)])
    s = (np.floor(s / h) + 0.5) * h
    s = np.unique(s, axis=0)
    pts = np.concatenate([g, w, s])
    pts = pts[rng.permutation(len(pts))]
    return np.column_stack([pts, rng.uniform(0.0, 1.0, len(pts))]), h, t


# name: (builder, arguments, K, seed); the runs of a case are (t, refine) pairs
CASES = {
    "slab 3": (slab, (3,), 8, 3),
    "slab 255": (slab, (255,), 64, 255),
    "slab 256": (slab, (256,), 64, 256),
    "slab 257": (slab, (257,), 64, 257),
    "slab 1281": (slab, (1281,), 100, 1281),          # 6 workgroup partials padded to 8
    "two equal planes": (two_planes, (), 200, 2),
    "collinear": (collinear, (), 50, 5),
    "dyadic edge": (dyadic_edge, (), 200, 7),
    "ground + wall": (ground_wall, (), 300, 11),
}
SLABS = tuple(name for name in CASES if name.startswith("slab"))

# The sizes at which the kernels and their host side change shape (module docstring), on h = 2^-6 so that the slab
# stays within its 64 metres.  Kept apart from CASES: the tests over CASES run several thresholds and hold the SLABS
# to margins that were worked out for h = 0.25.
TILE = 1024                         # csrc/plane.hpp kPlaneTile: voxels per workgroup and turn of the score kernel
SCORE_GRID = 2048                   # kPlaneScoreGrid: its workgroups at the most
TWO_TURNS = SCORE_GRID * TILE + TILE + 1          # 2 098 177: 2 050 tiles, the last of one voxel
LARGE = {
    "slab 32769": (slab, (32769, None, 2.0 ** -6), 64, 32769),
    "slab 65537": (slab, (65537, None, 2.0 ** -6), 64, 65537),
    f"slab {TWO_TURNS}": (slab, (TWO_TURNS, None, 2.0 ** -6), 8, 3),
}
_cache = {}


def _built(rows, h, t, K, seed, origin, one_each):
    d = V.downsample(rows, h, origin)
    assert not one_each or len(d["keys"]) == len(rows)             # one point per voxel
    return dict(rows=rows, h=h, origin=origin, t=t, K=K, seed=seed, vox=d, cent=np.ascontiguousarray(d["rows"][:, :3]))


def case(name, origin=V.ZERO):
    """-> dict(rows, h, origin, t, K, seed, vox = V.downsample(rows, h, origin), cent (M, 3)); nobody writes into it"""
    origin = tuple(float(v) for v in origin)
    key = name if origin == V.ZERO else ("case", name, origin)
    if key not in _cache:
        builder, args, K, seed = (CASES.get(name) or LARGE[name])
        rows, h, t = builder(*args)
        _cache[key] = _built(rows, h, t, K, seed, origin, origin == V.ZERO)
    return _cache[key]


def among_of(M):
    """The candidates the large cases run among: two voxels of every three."""
    return np.arange(M) % 3 != 0


def grid_case(grid, float32=False):
    """case()'s dict for slab(257) built with the h of V.ORIGIN_GRIDS[grid] (as many cells wide as at h = 0.25), where
    that grid has its cloud, on the grid's h and origin; K = 64, seed 257.  Off the default origin two points may
    share a voxel.  float32: the values a batch can hold."""
    key = ("grid", grid, float32)
    if key not in _cache:
        g = V.ORIGIN_GRIDS[grid]
        rows, h, t = slab(257, h=g["h"], extent=256 * g["h"])
        rows = V.on_grid(rows, grid)
        _cache[key] = _built(V.as_float32(rows) if float32 else rows, h, t, 64, 257, g["origin"], False)
    return _cache[key]


def grid_expect(grid, refine, float32=False):
    """The restatement of a grid case (shared: nobody writes into it)."""
    k = ("grid expect", grid, bool(refine), float32)
    if k not in _cache:
        c = grid_case(grid, float32)
        e = ransac(c["cent"], c["t"], c["K"], c["seed"], refine)
        e["cent"] = c["cent"]
        _cache[k] = e
    return _cache[k]


def thresholds(name):
    """The thresholds a case runs at."""
    t = case(name)["t"]
    return (t, float(np.nextafter(np.float64(t), 0.0))) if name == "dyadic edge" else (t,)


def expect(name, refine, t=None, K=None, among=None, key=None):
    """The restatement of a case (shared: nobody writes into it); key names a cached variant with among."""
    c = case(name)
    t = c["t"] if t is None else t
    K = c["K"] if K is None else K
    k = ("expect", name, bool(refine), float(t), K, key)
    assert among is None or key is not None
    if k not in _cache:
        e = ransac(c["cent"], t, K, c["seed"], refine, among)
        e["cent"] = c["cent"]
        _cache[k] = e
    return _cache[k]


def margin(e, t, cand=None):
    """The smallest | |s| - t | of a refined result over its candidates."""
    s = np.abs(e["offsets"]) if cand is None else np.abs(e["offsets"][cand])
    return float(np.abs(s - t).min())


def equal(got, want, refine):
    """A VoxelPlane (or the host harness's dict) against the restatement: the integers and masks equal, the unrefined
    model bit for bit; the refit through check_refit."""
    g = got._asdict() if hasattr(got, "_asdict") else got
    ok = (g["iteration"] == want["iteration"] and g["score"] == want["score"] and g["n_inliers"] == want["n_inliers"]
          and np.array_equal(g["samples"], want["samples"]) and np.array_equal(g["inliers"], want["inliers"])
          and bool(g["refined"]) == want["refined"])
    if not ok:
        return False
    if want["refined"]:
        check_refit(g["model"], g["covariance"], want, None)
    else:
        assert g["covariance"] is None or not np.any(g["covariance"])
        assert np.array_equal(np.asarray(g["model"]).view(np.uint64), want["model"].view(np.uint64)), (g["model"], want["model"])
    return True
