"""The rays through a voxel cloud restated in plain Python floats and ints: this project's own definition
(include/mcdeskew.h "rays through the voxel cloud"), which csrc/rays_core.hpp and the kernel of csrc/rays.hpp must
reproduce count for count.  One Python float operation is one IEEE float64 operation; the cloud is a dict from a
cell's key (kx, ky, kz) to its voxel id.

  cell(v, h, o)                 the filter's grid lines of one end of a ray -> (g, k), or None when it is refused
  walk(s, e, h, o, max_steps)   the cells of the ray s -> e, positions 0 .. steps, or None when the ray is skipped
  count(keys, h, o, src, origins, guard, max_steps)   passed, ended, through, n_rays, n_skipped, steps

CASES names the cases the CPU tests (tests/test_rays_cpu.py, on the host build of the core) and the GPU tests
(tests/test_gpu_rays.py, on the kernel) share; case(name) builds one: the grid, the rows the cloud is built from, the
source points, their sensor positions, guard and max_steps."""
import functools
import math

import numpy as np

import voxel as V

KEY_MIN, KEY_END = V.KEY_MIN, V.KEY_END
INF = math.inf


def cell(v, h, o):
    """The grid lines of a point: a = v - o; g = a / h; k = floor(g) per axis -> (g, k), None when voxel_quantise
    refuses it (a coordinate or g that is not finite, a key outside [-2^20, 2^20))."""
    g, k = [], []
    for a in range(3):
        va = float(v[a])
        d = va - float(o[a])
        ga = d / float(h)
        if not (math.isfinite(va) and math.isfinite(ga)):
            return None
        ka = math.floor(ga)
        if not KEY_MIN <= ka < KEY_END:
            return None
        g.append(ga)
        k.append(ka)
    return g, k


def walk(s, e, h, o, max_steps):
    """The cells of the ray s -> e in walk order, position 0 the origin's and the last the endpoint's; None: skipped."""
    cs, ce = cell(s, h, o), cell(e, h, o)
    if cs is None or ce is None:
        return None
    (gs, ks), (ge, ke) = cs, ce
    d = [ge[a] - gs[a] for a in range(3)]
    dirs = [1 if ke[a] > ks[a] else (-1 if ke[a] < ks[a] else 0) for a in range(3)]
    n = [abs(ke[a] - ks[a]) for a in range(3)]
    steps = n[0] + n[1] + n[2]
    if steps > max_steps:
        return None
    j = [0, 0, 0]

    def t(a):
        if j[a] == n[a]:
            return INF
        b = float(ks[a] + j[a] * dirs[a] + (1 if dirs[a] > 0 else 0))
        u = b - gs[a]
        return u / d[a]

    k = list(ks)
    cells = [tuple(k)]
    for _ in range(steps):
        ts = (t(0), t(1), t(2))
        a = 0
        if ts[1] < ts[a]:
            a = 1
        if ts[2] < ts[a]:
            a = 2
        k[a] += dirs[a]
        j[a] += 1
        cells.append(tuple(k))
    assert k == ke
    return cells


def count(keys, h, o, src, origins, guard, max_steps):
    """keys (M, 3) in the cloud's order; src (N, >= 3); origins (3,), (1, 3) or (N, 3) -> dict(passed (M,) int32,
    ended (M,) int32, through (N,) int32, n_rays, n_skipped, steps)."""
    vox = {tuple(int(x) for x in k): v for v, k in enumerate(np.asarray(keys).reshape(-1, 3))}
    assert len(vox) == len(keys)
    src = np.asarray(src, np.float64)
    org = np.asarray(origins, np.float64).reshape(-1, 3)
    assert len(org) in (1, len(src))
    passed, ended = np.zeros(len(vox), np.int32), np.zeros(len(vox), np.int32)
    through = np.zeros(len(src), np.int32)
    skipped = steps = 0
    for i in range(len(src)):
        cells = walk(org[i if len(org) > 1 else 0].tolist(), src[i, :3].tolist(), h, o, max_steps)
        if cells is None:
            through[i] = -1
            skipped += 1
            continue
        n = len(cells) - 1
        steps += n
        v = vox.get(cells[n])
        if v is not None:
            ended[v] += 1
        for c in cells[:max(n - guard, 0)]:              # positions 0 .. steps - 1 - guard
            v = vox.get(c)
            if v is not None:
                passed[v] += 1
                through[i] += 1
    return dict(passed=passed, ended=ended, through=through, n_rays=len(src), n_skipped=skipped, steps=steps)


def equal(got, want):
    """Every count, every `through` and the three stats."""
    return (all(np.array_equal(np.asarray(got[k], np.int32), want[k]) for k in ("passed", "ended", "through"))
            and all(int(got[k]) == want[k] for k in ("n_rays", "n_skipped", "steps")))


# ---- the cases ----------------------------------------------------------------------------------------------------
H = 0.5                                  # exact in binary: with the origin (0, 0, 0), g = v / h is exact on dyadic values
BOX = (-3, 8)                            # the cells of the cases' cloud on every axis: one voxel per cell of the box
BEYOND = 2.0 * KEY_END                   # a g no key can hold


def grid_of(name):
    """(h, origin, place): the default grid, or one of V.ORIGIN_GRIDS with the points moved where its cloud is."""
    if name is None:
        return H, V.ZERO, lambda p: np.array(p, np.float64)
    g = V.ORIGIN_GRIDS[name]
    return g["h"], g["origin"], lambda p: V.on_grid(p, name)


def at(g, h):
    """Grid units -> the coordinates the case is written in (before a moved grid moves them)."""
    return np.asarray(g, np.float64) * h


def box_rows(h, place, lo=BOX[0], hi=BOX[1]):
    """One point at the centre of every cell of the box, intensity 0.5."""
    k = np.arange(lo, hi, dtype=np.float64) + 0.5
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    rows = np.full((len(g), 4), 0.5)
    rows[:, :3] = place(at(g, h))
    return rows


def rays_case(grid, pairs, guard, max_steps=4096, rows=None):
    """pairs: (s, e) in grid units, one sensor position per ray."""
    h, origin, place = grid_of(grid)
    s = place(at([p[0] for p in pairs], h))
    e = place(at([p[1] for p in pairs], h))
    return dict(h=h, origin=origin, rows=box_rows(h, place) if rows is None else rows, src=e, origins=s, guard=guard,
                max_steps=max_steps)


C = (0.5, 0.5, 0.5)                      # the centre of cell (0, 0, 0)
AXIS = [(C, (5.5, 0.5, 0.5)), (C, (0.5, -2.5, 0.5)), (C, (0.5, 0.5, 6.5))]
# all three axes tie at every crossing; two axes tie; the same ties walked in the negative direction
TIES = [(C, (3.5, 3.5, 3.5)), (C, (3.5, 3.5, 0.5)), (C, (0.5, 3.5, 3.5)), ((3.5, 3.5, 3.5), C), ((3.5, 3.5, 0.5), C),
        ((3.5, 0.5, 3.5), C), ((3.5, 0.5, 0.5), (0.5, 3.5, 3.5))]
TIE_ORDER = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
# an endpoint, and an origin, with g an exact integer on one, two and three axes, approached from both sides
FACES = [(C, (3.0, 0.5, 0.5)), (C, (3.0, 2.0, 1.0)), ((3.5, 0.5, 0.5), (1.0, 0.5, 0.5)), ((3.5, 3.5, 3.5), (1.0, 2.0, 0.0)),
         ((2.0, 0.5, 0.5), (4.5, 2.5, 0.5)), ((2.0, 1.0, 3.0), (4.5, 2.5, 0.5)), ((2.0, 1.0, 3.0), (-0.5, -1.5, 0.5)),
         ((2.0, 2.0, 2.0), (5.0, 5.0, 5.0)), ((5.0, 5.0, 5.0), (2.0, 2.0, 2.0))]
SAME = [((0.25, 0.375, 0.5), (0.75, 0.625, 0.875)), (C, C), ((-1.0, -1.0, -1.0), (-0.5, -0.25, -0.125))]
# walks of 0, 1, 3 and 4 steps
BY_STEPS = [((0.25, 0.5, 0.5), (0.75, 0.5, 0.5)), ((0.25, 0.5, 0.5), (1.75, 0.5, 0.5)), ((0.25, 0.5, 0.5), (3.75, 0.5, 0.5)),
            ((0.25, 0.25, 0.5), (2.75, 2.5, 0.5)), ((0.25, 0.5, 0.5), (4.75, 0.5, 0.5)), ((4.25, 0.375, 0.5), (2.75, 2.625, 1.5))]
GOOD = [(C, (4.25, 2.5, 1.75)), ((-1.5, 2.25, 0.5), (6.5, -0.75, 3.25))]


def _negative_case():
    """The grid's origin at (-10, -10, -10): every coordinate of the case is negative, and both walks cross key 0 on
    every axis, one upwards and one downwards."""
    def place(p):
        return np.asarray(p, np.float64) - 10.0
    s = place(at([(-2.6, -1.6, -2.2), (2.6, 1.6, 2.2)], H))
    e = place(at([(2.2, 1.2, 1.6), (-0.4, -2.8, -1.2)], H))
    assert (s < 0).all() and (e < 0).all()
    return dict(h=H, origin=(-10.0, -10.0, -10.0), rows=box_rows(H, place), src=e, origins=s, guard=1, max_steps=4096)


def _skipped_case(origins_too):
    nan, inf = math.nan, math.inf
    e = (2.5, 1.5, 0.5)
    pairs = [GOOD[0], (C, (nan, 0.5, 0.5)), (C, (0.5, inf, 0.5)), (C, (0.5, 0.5, -inf)), (C, (BEYOND, 0.5, 0.5)),
             (C, (0.5, -BEYOND, 0.5)), GOOD[1], ((BEYOND, 0.5, 0.5), e), ((0.5, 0.5, -BEYOND), e), (C, (0.5, 0.5, float(KEY_END)))]
    if origins_too:      # what the module refuses of its origins and the library's rows entry point walks as skipped
        pairs += [((nan, 0.5, 0.5), e), ((0.5, -inf, 0.5), e), ((0.5, 0.5, inf), e), GOOD[0]]
    return rays_case(None, pairs, 1)


def _contention_case():
    """4097 rays from distinct sensor positions in cell (0, 0, 0) along +x: all pass (5, 0, 0) and end in (10, 0, 0)."""
    n = 4097
    s = np.full((n, 3), 0.5)
    s[:, 0] = 0.0625 + np.arange(n) * 2.0 ** -13
    e = np.tile([10.5, 0.5, 0.5], (n, 1))
    rows = np.full((3, 4), 0.5)
    rows[:, :3] = at([(5.5, 0.5, 0.5), (10.5, 0.5, 0.5), (0.5, 0.5, 0.5)], H)
    return dict(h=H, origin=V.ZERO, rows=rows, src=at(e, H), origins=at(s, H), guard=1, max_steps=4096)


FRAME_COUNTS = (0, 1, 255, 256, 257)


def _frames_case():
    """769 rays a batch can hold (float32 values) in frames of 0, 1, 255, 256 and 257 points, one sensor position per
    frame; `origins` is the per-row form, `frame_origins` the (F, 3) one."""
    rng = np.random.default_rng(11)
    n = sum(FRAME_COUNTS)
    e = V.as_float32(at(rng.uniform(-2.5, 7.5, (n, 3)), H))
    fo = V.as_float32(at(rng.uniform(-1.0, 6.0, (len(FRAME_COUNTS), 3)), H))
    c = dict(h=H, origin=V.ZERO, rows=box_rows(H, np.asarray), src=e, origins=np.repeat(fo, FRAME_COUNTS, axis=0), guard=1,
             max_steps=4096)
    c["frame_origins"], c["counts"] = fo, FRAME_COUNTS
    return c


def _own_points_case():
    """The cloud is built from the source itself: every ray ends in the voxel its point was put in."""
    rng = np.random.default_rng(12)
    e = rng.uniform(-4.0, 9.0, (500, 3)) * 0.37
    rows = np.full((len(e), 4), 0.25)
    rows[:, :3] = e
    return dict(h=0.1, origin=(0.013, -0.27, 1.1), rows=rows, src=e, origins=rng.uniform(-2.0, 2.0, (len(e), 3)), guard=1,
                max_steps=4096)


# A long ray on which the crossing parameters accumulated by adding 1 / |d| drift past a neighbour's: found by a search
# over seeded rays for the first whose accumulated walk leaves the restatement's (tests/test_rays_cpu.py asserts that it
# does).  The cloud holds exactly the cells of the restatement's walk.
LONG_S, LONG_E = (0.5, 0.8, 0.6), (1342.5, 1196.0, 394.2)      # 2932 steps; the accumulated walk leaves it at step 733


def accumulated_walk(s, e, h, o):
    """The walk with t_a advanced by t_a += 1 / |d_a| from its first crossing: what the definition forbids."""
    (gs, ks), (ge, ke) = cell(s, h, o), cell(e, h, o)
    d = [ge[a] - gs[a] for a in range(3)]
    dirs = [1 if ke[a] > ks[a] else (-1 if ke[a] < ks[a] else 0) for a in range(3)]
    left = [abs(ke[a] - ks[a]) for a in range(3)]
    t = [(float(ks[a] + (1 if dirs[a] > 0 else 0)) - gs[a]) / d[a] if left[a] else INF for a in range(3)]
    k = list(ks)
    cells = [tuple(k)]
    for _ in range(sum(left)):
        a = 0
        if t[1] < t[a]:
            a = 1
        if t[2] < t[a]:
            a = 2
        k[a] += dirs[a]
        left[a] -= 1
        t[a] = t[a] + 1.0 / abs(d[a]) if left[a] else INF
        cells.append(tuple(k))
    return cells


def _long_case():
    h, o = 0.1, (0.0, 0.0, 0.0)
    s, e = at([LONG_S], h), at([LONG_E], h)
    cells = np.array(walk(s[0].tolist(), e[0].tolist(), h, o, 4096), np.float64)
    rows = np.full((len(cells), 4), 0.5)
    rows[:, :3] = (cells + 0.5) * h
    return dict(h=h, origin=o, rows=rows, src=e, origins=s, guard=1, max_steps=4096)


# ---- the ghost: the known answer -------------------------------------------------------------------------------------
GHOST_H = 0.25
GHOST_ORIGIN = (0.125, 0.125, 1.125)     # the sensor, in the cloud's frame: the centre of a cell


def ghost():
    """A wall at x = 10 .. 10.25 (one cell thick, 24 x 12 cells, four points per cell) and a box of 3 x 4 x 3 cells of
    points in front of it at x = 5.  The scan sees the wall alone, from GHOST_ORIGIN.  -> (wall rows, box rows)."""
    q = np.array([0.0625, 0.1875])
    y = (np.arange(-12, 12)[:, None] * GHOST_H + q[None, :]).reshape(-1)
    z = (np.arange(0, 12)[:, None] * GHOST_H + q[None, :]).reshape(-1)
    yy, zz = np.meshgrid(y, z, indexing="ij")
    wall = np.stack([np.full(yy.size, 10.125), yy.reshape(-1), zz.reshape(-1), np.full(yy.size, 0.5)], axis=1)
    k = np.stack(np.meshgrid(np.arange(20, 23), np.arange(-2, 2), np.arange(3, 6), indexing="ij"), axis=-1).reshape(-1, 3)
    box = np.full((len(k), 4), 0.75)
    box[:, :3] = (k + 0.5) * GHOST_H
    return wall, box


def _ghost_case():
    wall, box = ghost()
    return dict(h=GHOST_H, origin=V.ZERO, rows=np.concatenate([wall, box]), src=wall[:, :3], origins=np.array(GHOST_ORIGIN),
                guard=1, max_steps=4096, wall=wall, box=box)


_BUILDERS = {
    "axis": lambda: rays_case(None, AXIS, 1),
    "diagonal ties": lambda: rays_case(None, TIES, 0),
    "negative keys": _negative_case,
    "on a face": lambda: rays_case(None, FACES, 1),
    "same cell, guard 0": lambda: rays_case(None, SAME, 0),
    "same cell, guard 1": lambda: rays_case(None, SAME, 1),
    "same cell, guard 255": lambda: rays_case(None, SAME, 255),
    "guard 0": lambda: rays_case(None, BY_STEPS, 0),
    "guard 1": lambda: rays_case(None, BY_STEPS, 1),
    "guard 3": lambda: rays_case(None, BY_STEPS, 3),
    # walks of 4, 5 and 6 steps at max_steps 5; of 0, 1 and 2 at max_steps 1
    "max_steps 5": lambda: rays_case(None, [BY_STEPS[4], ((0.25, 0.5, 0.5), (5.75, 0.5, 0.5)), ((0.25, 0.5, 0.5), (6.75, 0.5, 0.5)),
                                            BY_STEPS[3], ((0.25, 0.25, 0.5), (3.75, 2.5, 0.5))], 0, max_steps=5),
    "max_steps 1": lambda: rays_case(None, [BY_STEPS[0], BY_STEPS[1], ((0.25, 0.5, 0.5), (2.75, 0.5, 0.5)),
                                            ((0.25, 0.5, 0.5), (1.75, 1.5, 0.5))], 0, max_steps=1),
    "skipped": lambda: _skipped_case(False),
    "skipped origins": lambda: _skipped_case(True),
    "contention": _contention_case,
    "frames": _frames_case,
    "own points": _own_points_case,
    "long": _long_case,
    "ghost": _ghost_case,
    "empty cloud": lambda: rays_case(None, AXIS + [(C, (math.nan, 0.5, 0.5))], 1, rows=np.zeros((0, 4))),
}
for _g in V.ORIGIN_GRIDS:
    _BUILDERS[f"axis on {_g}"] = functools.partial(rays_case, _g, AXIS, 1)
    _BUILDERS[f"ties on {_g}"] = functools.partial(rays_case, _g, TIES, 0)

CASES = tuple(_BUILDERS)
# the sensor positions of this case are not finite: the module refuses them, the core and the library's rows entry
# point walk them as skipped rays
NOT_FINITE_ORIGINS = ("skipped origins",)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = _BUILDERS[name]()
    c["keys"] = V.downsample(c["rows"], c["h"], c["origin"])["keys"]
    return c


def case(name):
    """dict(h, origin, rows (the cloud's source), keys (the cloud's, in its order), src, origins, guard, max_steps)."""
    return dict(_case(name))


@functools.lru_cache(maxsize=None)
def expect(name):
    c = _case(name)
    return count(c["keys"], c["h"], c["origin"], c["src"], c["origins"], c["guard"], c["max_steps"])
