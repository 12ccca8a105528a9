"""The density clustering of a voxel cloud restated in NumPy and scipy: this project's own definition
(include/mcdeskew.h "density clustering of the voxel cloud"; csrc/cluster_core.hpp), which the kernels of
csrc/cluster.hpp must reproduce exactly — every output is an integer — and the clouds the tests run it on.

The neighbour relation is tests/normals.py's (estimate(..., max_nn=0): `kept` and `nbr` in walk order); on top of
it the density, the core set, scipy's connected components over the core-core edges, the border choice by
lexsort on (ix, d2), and the numbering by lowest core voxel id.  Nothing here shares code with the library."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import normals as N
import voxel as V


def dbscan(keys, cent, counts, h, eps, min_points, weighted=False, est=None):
    """keys (M, 3), cent (M, 3) float64, counts (M,) source points (V.downsample's keys, rows[:, :3], counts) ->
    dict(labels, density (M,) int32; K; voxels (K,) int32; points (K,) int64; cell_min, cell_max (K, 3) int32;
    core (M,) bool)."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    c = np.ascontiguousarray(np.asarray(cent, np.float64).reshape(-1, 3))
    counts = np.asarray(counts, np.int64)
    M = len(keys)
    if est is None:
        est = N.estimate(keys, c, h, eps, 0)
    nbr, kept = est["nbr"], est["kept"]
    w = counts if weighted else np.ones(M, np.int64)
    density = np.where(kept, w[np.maximum(nbr, 0)], 0).sum(axis=1)
    core = density >= min_points
    i, ix = np.nonzero(kept)
    j = nbr[i, ix]
    assert (j >= 0).all()
    e = core[i] & core[j]
    _, comp = connected_components(coo_matrix((np.ones(int(e.sum())), (i[e], j[e])), shape=(M, M)), directed=False)
    # a component's root: its lowest (core) voxel id
    low = np.full(M, M, np.int64)
    np.minimum.at(low, comp[core], np.flatnonzero(core))
    root = np.full(M, -1, np.int64)
    root[core] = low[comp[core]]
    # border voxels: the core neighbour of smallest (d2, ix)
    rest = np.flatnonzero(~core)
    ixs = np.arange(kept.shape[1])
    for at in range(0, len(rest), 2048):
        b = rest[at:at + 2048]
        jb = np.maximum(nbr[b], 0)
        ok = kept[b] & core[jb]
        u = c[jb] - c[b][:, None, :]
        xx = u[..., 0] * u[..., 0]
        yy = u[..., 1] * u[..., 1]
        zz = u[..., 2] * u[..., 2]
        xy = xx + yy
        d2 = np.where(ok, xy + zz, np.inf)
        best = np.lexsort((np.broadcast_to(ixs, d2.shape), d2), axis=-1)[:, 0]
        has = ok.any(axis=1)
        root[b[has]] = root[jb[has, best[has]]]
    roots = np.unique(root[root >= 0])
    labels = np.full(M, -1, np.int32)
    labels[root >= 0] = np.searchsorted(roots, root[root >= 0])
    K = len(roots)
    on = labels >= 0
    voxels = np.bincount(labels[on], minlength=K).astype(np.int32)
    points = np.zeros(K, np.int64)
    np.add.at(points, labels[on], counts[on])
    cell_min = np.full((K, 3), np.iinfo(np.int32).max, np.int64)
    cell_max = np.full((K, 3), np.iinfo(np.int32).min, np.int64)
    np.minimum.at(cell_min, labels[on], keys[on])
    np.maximum.at(cell_max, labels[on], keys[on])
    return dict(labels=labels, density=density.astype(np.int32), K=K, voxels=voxels, points=points,
                cell_min=cell_min.astype(np.int32), cell_max=cell_max.astype(np.int32), core=core)


FIELDS = ("labels", "density", "voxels", "points", "cell_min", "cell_max")


def equal(got, want):
    """got: a VoxelClusters or a dict as dbscan's; every array of the same dtype, shape and values, and K."""
    g = got if isinstance(got, dict) else dict(got._asdict(), K=got.n_clusters)
    return g["K"] == want["K"] and all(
        g[f].dtype == want[f].dtype and g[f].shape == want[f].shape and np.array_equal(g[f], want[f]) for f in FIELDS)


def canonical(labels, core):
    """Are the clusters numbered by the first appearance of their cores: cluster k's lowest core voxel id ascends with k, and every
    number below the highest has a core voxel?"""
    on = labels[core]
    if (on < 0).any():
        return False
    if not len(on):
        return bool((labels < 0).all())
    first = np.full(labels.max() + 1, len(labels), np.int64)
    np.minimum.at(first, on, np.flatnonzero(core))
    return bool((first < len(labels)).all() and (np.diff(first) > 0).all())


# ---- the clouds ------------------------------------------------------------------------------------------------
def centres(cells, h):
    cells = np.asarray(cells)
    return np.column_stack([(cells + 0.5) * h, np.full(len(cells), 0.5)])


TIE_A = [(x, y, z) for x in (-1, 0) for y in (-1, 0, 1) for z in (-1, 0, 1)]
TIE_B = [(x, y, z) for x in (4, 5) for y in (-1, 0, 1) for z in (-1, 0, 1)]
TIE_BETWEEN = (2, 0, 0)


def tie(b_first=False, border_first=False):
    """Two 2 x 3 x 3 blocks of exact-centre cells and one cell between them whose core neighbours (0, 0, 0) and
    (4, 0, 0) are both exactly eps away: -> rows, h = 0.5, eps = 1.0; at min_points = 4 the cell between has
    density 3 and must join block A, whose cell has the lower key, whichever block comes first.  border_first: the
    cell between comes before both blocks, so a border voxel has the lowest id of its cluster (clusters are numbered
    by their lowest core voxel id: B's, whose cores come first, is 0 and voxel 0 carries label 1)."""
    blocks = TIE_B + TIE_A if b_first else TIE_A + TIE_B
    return centres([TIE_BETWEEN] + blocks if border_first else blocks + [TIE_BETWEEN], 0.5), 0.5, 1.0


def chain_cells(n=5000, width=40):
    """A one-cell-wide serpentine in z = 0: rows of `width` cells along x joined by two-cell risers."""
    cells = []
    x = y = 0
    step = 1
    while len(cells) < n:
        for _ in range(width):
            cells.append((x, y, 0))
            x += step
        x -= step
        cells.append((x, y + 1, 0))
        cells.append((x, y + 2, 0))
        y += 3
        step = -step
    return np.array(cells[:n])


def chain():
    """The serpentine fed in reverse path order, so the ids descend along it (the deep-tree case of find):
    -> rows, h = 0.5, eps = 0.5; at min_points = 2 one cluster, no noise, densities 2 to 3."""
    return centres(chain_cells()[::-1], 0.5), 0.5, 0.5


def contention():
    """32 x 32 x 32 exact-centre cells in a seeded random order: -> rows, h = 0.5, eps = h, so R = 1 and each
    voxel has six neighbours at d2 == h * h exactly; at min_points = 1 one cluster of 32 768 voxels."""
    k = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij"), axis=-1).reshape(-1, 3)
    k = k[np.random.default_rng(32).permutation(len(k))]
    return centres(k, 0.5), 0.5, 0.5


def weighted_slab():
    """The 257-voxel slab with every point repeated 1 to 6 times (a repeated point leaves the centroid's bits
    alone): -> rows, h, eps = 2 h; the voxels hold 1 to 6 points."""
    rows, h, eps = N.slab(257, 257)
    reps = np.random.default_rng(6).integers(1, 7, len(rows))
    return np.repeat(rows, reps, axis=0), h, eps


def _normals_case(name):
    def build():
        c = N.case(name)
        return c["rows"], c["h"], c["radius"]
    return build


CASES = {
    # name: (builder -> rows, h, eps; the (min_points, weighted) it is run at)
    "tie": (tie, ((4, False),)),
    "tie, B first": (lambda: tie(True), ((4, False),)),
    "tie, border first": (lambda: tie(True, True), ((4, False),)),
    "isolated": (lambda: N.isolated(), ((3, False), (2, False))),
    "isolated, eps just under": (lambda: (*N.isolated()[:2], float(np.nextafter(1.0, 0))), ((3, False),)),
    "chain": (chain, ((2, False),)),
    "contention": (contention, ((1, False),)),
    "block": (lambda: N.block(), ((1, False),)),
    "30 voxels": (_normals_case("30 voxels"), ((1, False), (4, False), (10, False))),
    "257 voxels": (_normals_case("257 voxels"), ((1, False), (4, False), (10, False))),
    "70001 voxels": (_normals_case("70001 voxels"), ((1, False), (4, False), (10, False))),
    "R = 1": (_normals_case("R = 1"), ((1, False), (4, False), (10, False))),
    "R = 4": (_normals_case("R = 4"), ((1, False), (4, False), (10, False))),
    "key ends": (lambda: N.key_ends()[:3], ((1, False), (4, False), (10, False))),
    "weighted": (weighted_slab, ((10, False), (10, True))),
}
_cache = {}


def _built(rows, h, eps, runs, origin):
    d = V.downsample(rows, h, origin)
    return dict(rows=rows, h=h, origin=origin, eps=eps, runs=runs, vox=d, est=N.estimate(d["keys"], d["rows"][:, :3], h, eps, 0))


def case(name, origin=V.ZERO):
    """-> dict(rows, h, origin, eps, runs, vox = V.downsample(rows, h, origin), est = N.estimate(..., max_nn=0));
    computed once per session and shared (nobody writes into it)."""
    origin = tuple(float(v) for v in origin)
    key = name if origin == V.ZERO else ("case", name, origin)
    if key not in _cache:
        builder, runs = CASES[name]
        rows, h, eps = builder()
        _cache[key] = _built(rows, h, eps, runs, origin)
    return _cache[key]


GRID_RUNS = ((1, False), (4, False), (10, True))


def grid_case(grid, float32=False):
    """case()'s dict for N.grid_rows(grid) on the grid's h and origin (V.ORIGIN_GRIDS), eps = 2 h, runs GRID_RUNS."""
    key = ("grid", grid, float32)
    if key not in _cache:
        g = V.ORIGIN_GRIDS[grid]
        _cache[key] = _built(N.grid_rows(grid, float32), g["h"], 2 * g["h"], GRID_RUNS, g["origin"])
    return _cache[key]


def expect(name, min_points, weighted=False, c=None):
    """The restatement's result for a case at (min_points, weighted), computed once; c: a grid_case's dict, with
    `name` the key it is kept under."""
    key = (name, min_points, weighted)
    if key not in _cache:
        c = case(name) if c is None else c
        d = c["vox"]
        _cache[key] = dbscan(d["keys"], d["rows"][:, :3], d["counts"], c["h"], c["eps"], min_points, weighted, c["est"])
    return _cache[key]


def grid_expect(grid, min_points, weighted, float32=False):
    return expect(("grid", grid, float32), min_points, weighted, grid_case(grid, float32))


def all_runs():
    return [(name, mp, w) for name, (_, runs) in CASES.items() for mp, w in runs]
