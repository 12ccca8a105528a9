"""Growing a voxel cloud restated in NumPy (include/mcdeskew.h "growing a voxel cloud"): the records (keys, n, S, SI)
of a cloud and the rules of a call on them.  An item is a point or a record standing for n points of its voxel; items
that hold a key of the cloud add into its record, new keys follow in order of the lowest item that holds them, and a
refused call changes nothing.  ``finalise`` is tests/voxel.py's: after any sequence of calls, ``result()`` must equal
``voxel.downsample`` of the concatenated sources in every field."""
import numpy as np

import voxel as V

LIMIT = 1 << 31            # a cloud holds fewer points than this
LOG2_MIN, LOG2_MAX = 6, 32


def table_log2(M, n, log2cap):
    """The growth rule: M voxels, n items, a table of 2^log2cap slots (0: none) -> log2 of the slots afterwards."""
    if log2cap > 0 and M + n <= (1 << log2cap) // 2:
        return log2cap
    need = 2 * (M + n)
    l = LOG2_MIN
    while l < LOG2_MAX and (1 << l) < need:
        l += 1
    return max(l, log2cap)


def record_ok(key, n, S, SI):
    """One record, on Python ints."""
    top = int(n) << 32
    return (1 <= n < LIMIT and all(V.KEY_MIN <= int(k) < V.KEY_END for k in key) and all(0 <= int(s) <= top for s in S)
            and -top <= int(SI) <= top)


class Cloud:
    def __init__(self, h, origin=(0.0, 0.0, 0.0)):
        self.h, self.origin = h, origin
        self.keys, self.n = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
        self.S, self.SI = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
        self.N = 0

    def insert(self, rows):
        """Points (n, >= 4) -> the number of new voxels; raises V.Refused(lowest refused row)."""
        rows = np.asarray(rows, np.float64)
        K, Q, QI, bad = V.quantise(rows[:, :3], rows[:, 3], self.h, self.origin)
        if bad.any():
            raise V.Refused(int(np.flatnonzero(bad)[0]))
        return self._add(K, np.ones(len(K), np.int64), Q, QI)

    def merge(self, keys, n, S, SI):
        """Records -> the number of new voxels; raises V.Refused(lowest refused record)."""
        for i in range(len(keys)):
            if not record_ok(keys[i], n[i], S[i], SI[i]):
                raise V.Refused(i)
        return self._add(np.asarray(keys, np.int64).reshape(-1, 3), np.asarray(n, np.int64), np.asarray(S, np.int64).reshape(-1, 3),
                         np.asarray(SI, np.int64))

    def _add(self, K, n, Q, QI):
        if self.N + int(n.sum()) >= LIMIT:
            raise ValueError("2^31 points")
        M = len(self.keys)
        both = np.concatenate([self.keys, K])
        _, first, inv = np.unique(V.pack(both), return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")          # the cloud's voxels stay 0 .. M - 1: they come first
        rank = np.empty(len(first), np.int64)
        rank[order] = np.arange(len(first))
        vid = rank[inv.reshape(-1)][M:]
        grown = len(first) - M
        self.keys = both[first[order]]
        self.n = np.concatenate([self.n, np.zeros(grown, np.int64)])
        self.S = np.concatenate([self.S, np.zeros((grown, 3), np.int64)])
        self.SI = np.concatenate([self.SI, np.zeros(grown, np.int64)])
        np.add.at(self.n, vid, n)
        np.add.at(self.S, vid, Q)
        np.add.at(self.SI, vid, QI)
        self.N += int(n.sum())
        return grown

    def result(self):
        """As voxel.downsample's dict."""
        out = V.finalise(self.keys, self.S, self.SI, self.n, self.h, self.origin) if len(self.n) else np.zeros((0, 4))
        return dict(rows=out, counts=self.n.astype(np.int32), keys=self.keys.astype(np.int32), f32=out.astype(np.float32),
                    S=self.S.copy(), SI=self.SI.copy())


def records_of(d):
    """voxel.downsample's dict -> (keys, n, S, SI), what a merge takes."""
    return d["keys"], d["counts"].astype(np.int64), d["S"], d["SI"]
