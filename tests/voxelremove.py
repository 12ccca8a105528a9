"""Shrinking a voxel cloud restated in NumPy (include/mcdeskew.h "shrinking a voxel cloud"): tests/voxelinsert.py's
records with the way out.  ``remove`` takes whole voxels out and keeps the survivors' order; ``subtract`` takes items
out of their voxels' records, and a voxel whose count reaches 0 leaves as in ``remove``.  A refused call changes nothing
and raises ``voxel.Refused`` with the lowest refused item as ``index`` and the kind of refusal as ``reason``."""
import numpy as np

import voxel as V
import voxelinsert as VI

ITEM, MISSING, POINTS, REMAINDER = "item", "missing", "points", "remainder"      # MC_VOXEL_SUB_ITEM .. _REMAINDER: 1 .. 4
WHY = {ITEM: 1, MISSING: 2, POINTS: 3, REMAINDER: 4}


def table_shrink_log2(M_keep, log2cap):
    """The shrink rule: M_keep survivors in a table of 2^log2cap slots (0: none) -> log2 of the slots afterwards."""
    if log2cap <= 0 or M_keep >= (1 << log2cap) // 8:
        return log2cap
    l = VI.LOG2_MIN
    while l < log2cap and (1 << l) < 4 * M_keep:
        l += 1
    return l


def remainder_ok(n, S, SI):
    """What a subtraction may leave of a record, on Python ints."""
    n, S, SI = int(n), [int(s) for s in S], int(SI)
    if n < 0 or n >= VI.LIMIT:
        return False
    if n == 0:
        return all(s == 0 for s in S) and SI == 0
    top = n << 32
    return all(0 <= s <= top for s in S) and -top <= SI <= top


def refused(index, reason, key=None):
    e = V.Refused(index)
    e.reason, e.key = reason, key
    return e


class Cloud(VI.Cloud):
    def remove(self, mask):
        """A (M,) bool mask -> the number of voxels removed; the survivors keep their order."""
        mask = np.asarray(mask)
        assert mask.dtype == np.bool_ and mask.shape == (len(self.keys),)
        keep = ~mask
        self.keys, self.n, self.S, self.SI = self.keys[keep], self.n[keep], self.S[keep], self.SI[keep]
        self.N = int(self.n.sum())
        return int(mask.sum())

    def subtract(self, rows):
        """Points (n, >= 4) -> the number of voxels that emptied and left."""
        rows = np.asarray(rows, np.float64)
        K, Q, QI, bad = V.quantise(rows[:, :3], rows[:, 3], self.h, self.origin)
        return self._sub(K, np.ones(len(K), np.int64), Q, QI, bad)

    def subtract_records(self, keys, n, S, SI):
        """Records -> the number of voxels that emptied and left."""
        bad = np.array([not VI.record_ok(keys[i], n[i], S[i], SI[i]) for i in range(len(keys))], np.bool_)
        K = np.asarray(keys, np.int64).reshape(-1, 3).copy()
        K[bad] = 0
        return self._sub(K, np.asarray(n, np.int64), np.asarray(S, np.int64).reshape(-1, 3), np.asarray(SI, np.int64), bad)

    def _sub(self, K, n, Q, QI, bad):
        if len(K) == 0:
            return 0
        # validate: the lowest item the filter refuses or whose voxel the cloud lacks, nothing written
        packed = V.pack(self.keys) if len(self.keys) else np.zeros(0, np.int64)
        order = np.argsort(packed, kind="stable")
        item = V.pack(K)
        if len(packed):
            at = np.minimum(np.searchsorted(packed[order], item), len(packed) - 1)
            found = packed[order][at] == item
        else:
            at, found = np.zeros(len(item), np.int64), np.zeros(len(item), np.bool_)
        wrong = bad | ~found
        if wrong.any():
            i = int(np.flatnonzero(wrong)[0])
            raise refused(i, ITEM if bad[i] else MISSING)
        points = int(n.sum())
        if points > self.N:
            raise refused(-1, POINTS)
        vid = order[at]
        cn, cS, cSI = self.n.copy(), self.S.copy(), self.SI.copy()
        np.subtract.at(cn, vid, n)
        np.subtract.at(cS, vid, Q)
        np.subtract.at(cSI, vid, QI)
        # check: the lowest item whose voxel is left with what no set of points sums to
        touched, lowest = np.unique(vid, return_index=True)
        wrong = [int(i) for v, i in zip(touched, lowest) if not remainder_ok(cn[v], cS[v], cSI[v])]
        if wrong:
            raise refused(min(wrong), REMAINDER, tuple(int(k) for k in self.keys[vid[min(wrong)]]))
        self.n, self.S, self.SI = cn, cS, cSI
        gone = self.n == 0
        self.keys, self.n, self.S, self.SI = self.keys[~gone], self.n[~gone], self.S[~gone], self.SI[~gone]
        self.N -= points
        return int(gone.sum())
