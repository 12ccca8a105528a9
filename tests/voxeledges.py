"""Shared builders of the voxel filter's edge tests (tests/test_voxel_edges_cpu.py,
tests/test_gpu_voxel_edges.py): numpy only, deterministic seeds.

Each builder aims at one place where the kernels of csrc/voxel.hpp can go wrong without the cases of
tests/test_gpu_voxel.py noticing; the condition that makes a builder's case bite is asserted on the
restatement alone in test_voxel_edges_cpu.py, and the GPU tests compare with tests/voxel.py only.

  scan_case        k_vox_scan past its first pass of 256 chunks: first appearances in every pass
  probe_case       probe chains that wrap from slot ``mask`` to slot 0 and are hundreds of slots long
                   (``slot_first`` restates voxel_slot_first, ``probe_model`` is linear probing in
                   index order)
  big_sum_case     per-voxel sums past 2^53, odd: double(S) is inexact
  frame_run_*      about 900 frames with runs of empty frames at both ends and around a one-point frame
  fuzz_case        random grids (h over five decades, origins up to UTM scale)
  own_voxel_rows   every point its own voxel (M = n)
"""
import functools

import numpy as np

import voxel as V

CHUNK = 2048                     # kVoxChunk: points per workgroup of the rank kernels
PASS = 256 * CHUNK               # points per pass of k_vox_scan
SCAN_SIZES = (PASS, PASS + 1, 2 * PASS + 3 * CHUNK + 17)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def frozen(a):
    a.setflags(write=False)
    return a


def table_log2(n):
    """log2 of the slots mc_voxel_build_* takes for n points: a power of two >= 2 n, 64 at the least."""
    log2cap = 6
    while (1 << log2cap) < 2 * n:
        log2cap += 1
    return log2cap


# ---- A: the rank scan across passes ------------------------------------------------------------------------
def uneven_counts(n, frames=11, empty=4, seed=0):
    """``frames`` uneven frame sizes summing to n, frame ``empty`` empty, no other ending on a 256-point block."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 1.8, frames)
    w[empty] = 0.0
    c = np.floor(w / w.sum() * n).astype(np.int64)
    live = [f for f in range(frames) if f != empty]
    c[live[-1]] += n - c.sum()
    while True:
        on_edge = [f for f in live if c[f] % 256 == 0]
        if not on_edge:
            return c
        f = on_edge[0]
        c[f] -= 1
        c[live[(live.index(f) + 1) % len(live)]] += 1


@functools.lru_cache(maxsize=None)
def scan_case(n):
    """-> (counts, rows (n, 4) holding float32 values, h): new voxels keep first-appearing through the
    whole index range (point i picks among the first i / 5 of 200 000 centres), and the last point
    opens a voxel of its own."""
    rng = np.random.default_rng(n)
    centre = rng.integers(-150, 150, (200000, 3))
    pick = np.minimum(rng.integers(0, 200000, n), np.arange(n) // 5)
    rows = f32(np.column_stack([(centre[pick] + rng.uniform(0.05, 0.95, (n, 3))) * 0.2, rng.uniform(0, 1, n)]))
    rows[-1, :3] = f32((np.array([200.0, -200.0, 200.0]) + 0.5) * 0.2)
    return frozen(uneven_counts(n, seed=n)), frozen(rows), 0.2


@functools.lru_cache(maxsize=None)
def scan_want(n):
    _, rows, h = scan_case(n)
    return V.downsample(rows, h)


def first_appearances(rows, h, origin=(0.0, 0.0, 0.0)):
    """The sorted indices of the points that are the first of their voxel."""
    K = V.quantise(rows[:, :3], rows[:, 3], h, origin)[0]
    return np.sort(np.unique(V.pack(K), return_index=True)[1])


# ---- B: long and wrapping probe chains ---------------------------------------------------------------------
FIB = np.uint64(0x9E3779B97F4A7C15)
NO_SLOT = 0xFFFFFFFF


def slot_first(keys, log2cap):
    """voxel_slot_first (csrc/voxel_core.hpp) of packed keys in a table of 2^log2cap slots."""
    at = ((np.asarray(keys, np.uint64) * FIB) >> np.uint64(64 - log2cap)) & np.uint64((1 << log2cap) - 1)
    at = at.astype(np.int64)
    at[at == NO_SLOT] = 0
    return at


def slot_next(at, log2cap):
    n = (at + 1) & ((1 << log2cap) - 1)
    return 0 if n == NO_SLOT else n


def probe_model(keys, log2cap):
    """Linear probing of the packed keys (one per point) in index order -> (occupied slots as a set,
    the steps each point walks beyond its first slot)."""
    table = [None] * (1 << log2cap)
    steps = np.zeros(len(keys), np.int64)
    for i, (key, at) in enumerate(zip(np.asarray(keys).tolist(), slot_first(keys, log2cap).tolist())):
        n = 0
        while table[at] is not None and table[at] != key:
            at = slot_next(at, log2cap)
            n += 1
        table[at] = key
        steps[i] = n
    return {s for s, k in enumerate(table) if k is not None}, steps


def cube_keys():
    """The 64^3 voxel indices of the cube [-32, 32)^3."""
    a = np.arange(-32, 32)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)


def chain_keys(log2cap, lowest, count, seed):
    """``count`` distinct voxel indices of the cube whose first slot in a 2^log2cap table is >= lowest,
    in a seeded order -> (k (count, 3), how many the cube holds)."""
    k = cube_keys()
    hit = np.flatnonzero(slot_first(V.pack(k), log2cap) >= lowest)
    return k[np.random.default_rng(seed).permutation(hit)[:count]], len(hit)


PROBE_CASES = ("one point per key", "four points per key", "64 slots")


@functools.lru_cache(maxsize=None)
def probe_case(which):
    """-> (counts, rows holding float32 values, h, voxel index of every point (n, 3)).  All values are
    dyadic, so the rows are exact in float32 and the keys are the ones chosen."""
    rng = np.random.default_rng(100 + which)
    if which == 0:      # 2048 keys, one point each: 4096 slots, every first slot in [4000, 4096)
        k, _ = chain_keys(12, 4000, 2048, 11)
        counts, h = [2048], 0.5
    elif which == 1:    # 512 such keys, four points each; every repetition in another order, two per frame
        keys, _ = chain_keys(12, 4000, 512, 12)
        k = np.concatenate([keys[rng.permutation(512)] for _ in range(4)])
        counts, h = [1024, 1024], 0.25
    else:               # the 64-slot minimum table: 32 keys whose first slot is in [60, 64)
        k, _ = chain_keys(6, 60, 32, 13)
        counts, h = [32], 1.0
    u = rng.integers(1, 8, (len(k), 3)) / 8.0
    rows = np.column_stack([(k + u) * h, rng.integers(0, 256, len(k)) / 256.0])
    assert np.array_equal(rows, f32(rows))
    return counts, frozen(rows), h, frozen(k)


# ---- C: sums past 2^53 -------------------------------------------------------------------------------------
BIG_N = 2200001                  # points per voxel: more than 2^21, so n * 2^32 passes 2^53


def big_sum_case():
    """-> (rows (2 BIG_N, 4) float64, h, origin): voxels (0, 0, 0) (even rows) and (1, 1, 0) (odd rows).
    Built anew on every call (140 MB are not worth keeping); the restatement of it is kept."""
    x = 1.0 - 2.0 ** -32
    top = (2.0 ** 32 - 1) / 2.0 ** 16
    rows = np.empty((2 * BIG_N, 4))
    rows[0::2] = [x, x - 2.0 * 2.0 ** -32, 0.5, top]
    rows[1::2] = [x + 1.0, 1.25, 0.75, -top]
    return frozen(rows), 1.0, (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def big_sum_want():
    rows, h, o = big_sum_case()
    return V.downsample(rows, h, o)


# ---- D: many frames, runs of empty frames ------------------------------------------------------------------
CYCLE = (0, 1, 3, 256, 0, 0, 513, 255, 257)


def frame_run_counts():
    """910 frames: two empty, 50 cycles, a one-point frame between two empty frames on either side, 50
    cycles, three empty."""
    return np.array([0, 0] + list(CYCLE) * 50 + [0, 0, 1, 0, 0] + list(CYCLE) * 50 + [0, 0, 0], np.int64)


@functools.lru_cache(maxsize=None)
def frame_run_rows(one_voxel):
    n = int(frame_run_counts().sum())
    rng = np.random.default_rng(40 + one_voxel)
    rows = f32(rng.uniform(0.05, 0.95, (n, 4)))
    if not one_voxel:
        rows[:, :3] = f32(rng.uniform(-3.0, 3.0, (n, 3)))
    return frozen(rows), (1.0 if one_voxel else 0.5)


def refusal_places():
    """name -> (frame, point within the frame, dense index)."""
    counts = frame_run_counts()
    off = np.concatenate([[0], np.cumsum(counts)])
    live = np.flatnonzero(counts)
    lone = 2 + 9 * 50 + 2
    big = int(np.flatnonzero(counts == 513)[37])
    places = {"first point of the first non-empty frame": (int(live[0]), 0),
              "last point of the last non-empty frame": (int(live[-1]), int(counts[live[-1]]) - 1),
              "one-point frame between empty frames": (lone, 0),
              "point 255 of a 513-point frame": (big, 255),
              "point 256 of a 513-point frame": (big, 256),
              "point 512 of a 513-point frame": (big, 512)}
    return {name: (f, i, int(off[f]) + i) for name, (f, i) in places.items()}


REFUSED_ROWS = ([np.nan, 0.5, 0.5, 0.5], [0.5, np.inf, 0.5, 0.5], [0.5, 0.5, -3.0e6, 0.5], [0.5, 0.5, 0.5, 65537.0],
                [0.5, 0.5, 0.5, np.nan], [3.0e6, 0.5, 0.5, 0.5])


# ---- E: grid fuzz ------------------------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(24))
FUZZ_COUNTS = (1000, 0, 2000, 1096)


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    """-> (h, origin, rows64, rows32): 4096 points o + (k + u) h in float64, and their float32 roundings.
    Half the k come from 256 indices within +-8, half from 700 indices uniform in +-R: R = 2^19 where
    float32 resolves h at that origin, else 2^10 (there the float32 values of the far points coincide
    in runs, and the voxels they share sit far from the origin)."""
    rng = np.random.default_rng(7000 + seed)
    h = float(10.0 ** rng.uniform(-3.0, 2.0))
    scale = (0.0, 1.0e3, 5.0e6)[seed % 3]
    o = scale * rng.uniform(-1.0, 1.0, 3)
    R = 1 << 19
    if np.spacing(np.float32(np.abs(o).max() + R * h)) > h / 4:
        R = 1 << 10
    near = rng.integers(-8, 9, (256, 3))
    far = rng.integers(-R, R, (700, 3))
    k = np.concatenate([near[rng.integers(0, 256, 2048)], far[rng.integers(0, 700, 2048)]])[rng.permutation(4096)]
    rows64 = np.column_stack([o + (k + rng.uniform(0.0, 1.0, (4096, 3))) * h, rng.uniform(0.0, 255.0, 4096)])
    return h, tuple(o.tolist()), frozen(rows64), frozen(f32(rows64))


# ---- F: every point its own voxel --------------------------------------------------------------------------
OWN_SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1023, 1025)


def own_voxel_rows(n, h=0.25, origin=(0.0, 0.0, 0.0), seed=None):
    """-> (rows holding float32 values, the voxel index of every row): n distinct voxels; h and origin
    dyadic, so the values are exact."""
    rng = np.random.default_rng(n if seed is None else seed)
    i = rng.permutation(n)
    keys = np.stack([i % 13 - 6, (i // 13) % 17 - 8, i // 221 - 4], axis=1)
    rows = np.column_stack([np.asarray(origin) + (keys + rng.integers(1, 8, (n, 3)) / 8.0) * h, rng.integers(0, 256, n) / 256.0])
    assert np.array_equal(rows, f32(rows))
    return rows, keys
