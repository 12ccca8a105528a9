"""Voxel-grid downsampling on the device (build-added; csrc/voxel_core.hpp,
csrc/voxel.hpp; include/mcdeskew.h ``mc_voxel_*``): the step after a global deskew, when the frames
of a drive are accumulated into one cloud and most points re-observe the same surfaces.

  voxel_downsample(batch_or_rows, voxel, origin=(0, 0, 0))  -> VoxelCloud
  VoxelCloud.n_voxels, .batch(), .rows(), .point_counts(), .keys(), .close()

One output point per occupied voxel: the mean of the voxel's points and of their intensities.  The
per-voxel sums are integers (the coordinate inside its voxel in 2^-32 voxel units, the intensity in
2^-16), so the result is the same bit for bit on every run, whatever order the atomics arrive in.
Values, op for op in float64 (each line one IEEE operation):

  a = double(v) - o    g = a / h    k = floor(g)    f = g - k    Q = int64(rint(f * 2^32))
  QI = int64(rint(double(intensity) * 2^16))
  m = double(sum Q) / double(n)    w = double(k) + m * 2^-32    c = o + w * h
  i = (double(sum QI) / double(n)) * 2^-16

|c - mean| <= h * 2^-32 plus float64 rounding; the intensity is within 2^-17 of the mean.  Voxels come
out in order of first appearance (for a batch: frame-major, then the index within the frame).  With
the default origin the grids of different calls coincide.

Refused, never dropped silently: a coordinate or (v - o) / h that is not finite, a voxel index
outside [-2^20, 2^20), an intensity that is not finite or beyond +-65536 — ValueError naming the
lowest refused point (frame and index for a batch, the row for rows), and nothing is returned.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_double, c_int32, c_int64

import numpy as np

from ._lib import check, ptr
from .runtime import Batch, Context, default_context

MAX_POINTS = 2 ** 31 - 1


def _grid(voxel, origin):
    """(h, origin as 3 float64), checked before a device is touched."""
    try:
        h = float(voxel)
    except (TypeError, ValueError):
        raise ValueError(f"voxel must be a number > 0, got {voxel!r}") from None
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"voxel must be finite and > 0, got {voxel!r}")
    o = np.ascontiguousarray(origin, dtype=np.float64)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"origin must be three finite numbers, got {origin!r}")
    return h, o


class VoxelCloud:
    """What the last :func:`voxel_downsample` of a context left on the device.  The outputs are produced
    on demand from the per-voxel sums, any number of times; the next ``voxel_downsample`` on the same
    context (or :meth:`close`) ends this object's validity."""

    def __init__(self, ctx: Context, n_voxels: int, generation: int):
        self.ctx, self.n_voxels, self._gen = ctx, int(n_voxels), generation

    def _live(self):
        if self.ctx._voxel_gen != self._gen:
            raise ValueError("this VoxelCloud is closed or was replaced by a later voxel_downsample on its context")

    def batch(self, with_pcd_len: bool = False) -> Batch:
        """A one-frame float32 Batch of the voxel points (x, y, z, intensity; no time column), ready for
        encode_pcd / write_las / the LVX writers.  ``with_pcd_len``: its text sums exist but are stale."""
        self._live()
        out = Batch(self.ctx, [self.n_voxels], with_pcd_len=with_pcd_len)
        check(self.ctx.lib.mc_voxel_emit_batch(self.ctx.handle, out.handle), "voxel_downsample")
        return out

    def _emit(self, dtype, width, which):
        self._live()
        if self.n_voxels == 0:
            return np.zeros((0, width) if width > 1 else (0,), dtype)
        n = self.n_voxels * width
        buf = self.ctx.device_buffer(n * np.dtype(dtype).itemsize)
        try:
            args = [None, None, None]
            args[which] = buf.ptr
            check(self.ctx.lib.mc_voxel_emit_f64(self.ctx.handle, *args), "voxel_downsample")
            a = buf.to_host(dtype, count=n)
        finally:
            buf.close()
        return a.reshape(self.n_voxels, width) if width > 1 else a

    def rows(self) -> np.ndarray:
        """(M, 4) float64: cx, cy, cz, intensity."""
        return self._emit(np.float64, 4, 0)

    def point_counts(self) -> np.ndarray:
        """(M,) int32: the points of each voxel."""
        return self._emit(np.int32, 1, 1)

    def keys(self) -> np.ndarray:
        """(M, 3) int32: kx, ky, kz."""
        return self._emit(np.int32, 3, 2)

    def close(self):
        """Give the filter's device scratch back (a later call allocates it again)."""
        if self.ctx._voxel_gen == self._gen:
            self.ctx._voxel_gen = None
            check(self.ctx.lib.mc_voxel_release(self.ctx.handle), "voxel close")


def voxel_downsample(src, voxel, origin=(0.0, 0.0, 0.0), context: Context | None = None) -> VoxelCloud:
    """Voxel-grid filter of ``src``: a device :class:`Batch` (its float32 points, frame-major) or host
    float64 rows (N, >= 4) = x, y, z, intensity, uploaded first.  Raises ValueError naming the lowest
    refused point (module docstring)."""
    h, o = _grid(voxel, origin)
    m = c_int64(0)
    if isinstance(src, Batch):
        ctx = src.ctx
        if context is not None and context is not ctx:
            raise ValueError("the batch belongs to another context")
        if src.n_points > MAX_POINTS:
            raise ValueError(f"{src.n_points} points: the voxel filter takes fewer than 2^31")
        ctx._voxel_gen = None
        bf, bi = c_int32(-1), c_int64(-1)
        check(ctx.lib.mc_voxel_build_batch(ctx.handle, src.handle, h, ptr(o, c_double), ctypes.byref(m),
                                           ctypes.byref(bf), ctypes.byref(bi)), "voxel_downsample")
    else:
        a = np.asarray(src)
        if a.ndim != 2 or a.shape[1] < 4:
            raise ValueError(f"rows must be (N, >= 4) = x, y, z, intensity; got shape {a.shape}")
        if a.shape[0] > MAX_POINTS:
            raise ValueError(f"{a.shape[0]} points: the voxel filter takes fewer than 2^31")
        ctx = context or default_context()
        a = np.ascontiguousarray(a, dtype=np.float64)
        ctx._voxel_gen = None
        d_rows = ctx.device_buffer(max(a.nbytes, 8))
        try:
            if a.size:
                d_rows.from_host(a)
            bad = c_int64(-1)
            check(ctx.lib.mc_voxel_build_f64(ctx.handle, d_rows.ptr, a.shape[1], a.shape[0], h, ptr(o, c_double),
                                             ctypes.byref(m), ctypes.byref(bad)), "voxel_downsample")
        finally:
            d_rows.close()
    ctx._voxel_serial += 1
    ctx._voxel_gen = ctx._voxel_serial
    return VoxelCloud(ctx, m.value, ctx._voxel_gen)
