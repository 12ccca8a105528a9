"""The kept normals of a voxel cloud restated in NumPy (include/mcdeskew.h "kept normals"): the cloud as its exact
records, its four edits, and for every edit the touched voxels T, the dirty set D and the cloud afterwards, on top of
tests/voxel.py and tests/normals.py.

  T   insert / merge: every voxel that received an item, new ones included; subtract: every voxel that lost one, emptied
      ones included; remove: the removed voxels
  D   the voxels present after the edit whose cell is within R = ceil(radius / h) cells, on every axis, of the cell of
      a touched voxel

The contract is that the rows of D computed again, with every other row carried over (on a removal to its new id), are
the fresh estimate of the edited cloud: patch() does exactly that to a stale estimate, and nothing more."""
from typing import NamedTuple

import numpy as np

import normals as N
import voxel as V

FIELDS = ("counts", "cov", "kept")      # what N.estimate returns per voxel: the normal is a function of these


class Cloud:
    """The records of a voxel cloud in its order: keys (M, 3), n (M,), S (M, 3), SI (M,), all int64."""

    def __init__(self, h, origin, keys, n, S, SI):
        self.h, self.origin = h, tuple(float(v) for v in origin)
        self.keys = np.asarray(keys, np.int64).reshape(-1, 3)
        self.n = np.asarray(n, np.int64).reshape(-1)
        self.S = np.asarray(S, np.int64).reshape(-1, 3)
        self.SI = np.asarray(SI, np.int64).reshape(-1)

    @classmethod
    def of_rows(cls, rows, h, origin=V.ZERO):
        d = V.downsample(np.asarray(rows, np.float64).reshape(-1, 4), h, origin)
        return cls(h, origin, d["keys"], d["counts"], d["S"], d["SI"])

    def __len__(self):
        return len(self.keys)

    def rows(self):
        return V.finalise(self.keys, self.S, self.SI, self.n, self.h, self.origin) if len(self) else np.zeros((0, 4))

    def estimate(self, radius, max_nn):
        return N.estimate(self.keys, self.rows()[:, :3], self.h, radius, max_nn)

    def records(self, ids):
        """The records of these voxels as items of a merge or of a subtraction: (keys, n, S, SI)."""
        ids = np.asarray(ids, np.int64)
        return self.keys[ids], self.n[ids], self.S[ids], self.SI[ids]


class Edit(NamedTuple):
    after: Cloud
    touched: np.ndarray     # (t, 3) the cells of T, each once
    carry: np.ndarray       # (M',) the id a voxel of `after` had before the edit, -1 for a new voxel


def items_of_rows(cloud, rows):
    """The points of rows as items on the cloud's grid: (keys, n = 1, Q, QI)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    K, Q, QI, bad = V.quantise(rows[:, :3], rows[:, 3], cloud.h, cloud.origin)
    assert not bad.any()
    return K, np.ones(len(K), np.int64), Q, QI


def _unique_cells(K):
    return np.unique(np.asarray(K, np.int64).reshape(-1, 3), axis=0)


def add(cloud, items):
    """insert (items_of_rows) or merge (records): every item into its voxel, new voxels in the order of the items."""
    K, n, Q, QI = (np.asarray(a, np.int64) for a in items)
    at = {int(p): i for i, p in enumerate(V.pack(cloud.keys))} if len(cloud) else {}
    keys, cn, S, SI = list(cloud.keys), list(cloud.n), list(cloud.S), list(cloud.SI)
    for k, m, q, qi, p in zip(K, n, Q, QI, V.pack(K) if len(K) else []):
        i = at.setdefault(int(p), len(keys))
        if i == len(keys):
            keys.append(k)
            cn.append(0)
            S.append(np.zeros(3, np.int64))
            SI.append(0)
        cn[i] += m
        S[i] = S[i] + q
        SI[i] += qi
    after = Cloud(cloud.h, cloud.origin, np.array(keys).reshape(-1, 3), cn, np.array(S).reshape(-1, 3), SI)
    carry = np.concatenate([np.arange(len(cloud)), np.full(len(after) - len(cloud), -1)]).astype(np.int64)
    return Edit(after, _unique_cells(K), carry)


def subtract(cloud, items):
    """Every item out of its voxel (which the cloud must hold); the voxels left without points leave, the others keep
    their order."""
    K, n, Q, QI = (np.asarray(a, np.int64) for a in items)
    at = {int(p): i for i, p in enumerate(V.pack(cloud.keys))}
    cn, S, SI = cloud.n.copy(), cloud.S.copy(), cloud.SI.copy()
    for m, q, qi, p in zip(n, Q, QI, V.pack(K) if len(K) else []):
        i = at[int(p)]
        cn[i] -= m
        S[i] -= q
        SI[i] -= qi
    assert (cn >= 0).all()
    stay = np.flatnonzero(cn > 0)
    assert (S[cn == 0] == 0).all() and (SI[cn == 0] == 0).all()
    return Edit(Cloud(cloud.h, cloud.origin, cloud.keys[stay], cn[stay], S[stay], SI[stay]), _unique_cells(K), stay)


def remove(cloud, mask):
    mask = np.asarray(mask, bool)
    stay = np.flatnonzero(~mask)
    return Edit(Cloud(cloud.h, cloud.origin, cloud.keys[stay], cloud.n[stay], cloud.S[stay], cloud.SI[stay]),
                cloud.keys[mask].reshape(-1, 3), stay)


def dirty(edit, R):
    """D: the ids, ascending, of the voxels of edit.after within R cells on every axis of a touched cell."""
    k, t = edit.after.keys, edit.touched
    if len(k) == 0 or len(t) == 0:
        return np.zeros(0, np.int64)
    hit = np.zeros(len(k), bool)
    for t0 in range(0, len(t), 256):                  # (M, 256, 3) at a time
        hit |= (np.abs(k[:, None, :] - t[None, t0:t0 + 256, :]).max(axis=2) <= R).any(axis=1)
    return np.flatnonzero(hit)


def patch(stale, fresh, edit, D):
    """The estimate before the edit with the rows of D (ids of edit.after) taken from `fresh` and every other row
    carried to its id after the edit.  A voxel that is new and not in D would have no row: that is a failure of D."""
    D = np.asarray(D, np.int64)
    out = {}
    for f in FIELDS:
        a = np.zeros_like(fresh[f])
        old = edit.carry >= 0
        a[old] = stale[f][edit.carry[old]]
        if f == "counts":
            a[~old] = -1                              # no row: equal to nothing
        a[D] = fresh[f][D]
        out[f] = a
    return out


def same(a, b):
    """Two estimates equal in every bit of every field."""
    return all(a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes() for f in FIELDS)


def cells_rows(cells, h, rng=None, origin=V.ZERO, spread=0.3):
    """One point in each cell: at its centre, or (rng) within `spread` of it in units of h on every axis."""
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    off = 0.5 if rng is None else 0.5 + rng.uniform(-spread, spread, cells.shape)
    pts = (cells + off) * h + np.asarray(origin, np.float64)
    return np.column_stack([pts, np.full(len(cells), 0.5) if rng is None else rng.uniform(0.0, 1.0, len(cells))])


def sheet(M, seed, h=0.25, thick=2):
    """M voxels of one random point each in distinct random cells of a slab `thick` cells thick, about a third
    occupied: a cloud whose windows hold a few dozen voxels at R = 2.  -> rows"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(M * 3.0 / thick)))
    cell = rng.permutation(side * side * thick)[:M]
    k = np.stack([cell // (side * thick) - side // 2, (cell // thick) % side - side // 2, cell % thick], axis=1)
    return cells_rows(k, h, rng)
